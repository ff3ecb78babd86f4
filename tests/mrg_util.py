"""Shared by the MRG31k3p tests and tools/gen_mrg_golden.py: the fixtures under tests/golden/mrg,
the case tables, the one-node plans and the state makers.

Everything here is compared bit for bit (``np.array_equal`` on the samples AND on the returned
state): ``mrg_uniform`` is 32-bit integer arithmetic, one conversion and one multiplication;
``MultinomialFromUniform`` / ``ChoiceFromUniform`` are sequential sums in the reference's order.  The
stored results are those of the reference's C implementations.

The state makers restate ``MRG_RandomStream.get_substream_rstates`` (sandbox/rng_mrg.py:814: row i is
row i-1 jumped 2^72 steps) and the step itself in plain Python integers; the generator holds both to
the reference before it writes anything.
"""
import glob
import json
import os

import numpy as np

from aesara_amd.plan import Node, Plan

MRG_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mrg")
DTYPES = ("float32", "float64")
PARTS = (1, 2, 3, 16, 64)
M1, M2 = 2147483647, 2147462579
SEED = 12345
EDGE_STATES = ([M1 - 1] * 3 + [M2 - 1] * 3, [1, 0, 0, 0, 0, 1], [0, 0, 1, 1, 0, 0])
FILE_MAX = 190_000          # bytes of one fixture file: larger arrays are cut into row chunks

# name -> (n_streams, size, options).  Options: "edge" (the first rows are EDGE_STATES), "symbolic"
# (size is a run-time input), "inplace", "calls" (consecutive draws, the state fed back).
# (n_streams, n_elements) are the smallest pairs that reach each seam: one stream; fewer samples than
# streams (untouched streams); exactly one each; one more; a remainder; below / at / above one
# wavefront; more than one workgroup; the reference's stream cap with a remainder.
UNIFORM_CASES = {
    "s1_1": (1, (1,), {}),
    "s1_37": (1, (37,), {}),
    "s5_3": (5, (3,), {}),
    "s5_5": (5, (5,), {}),
    "s5_6": (5, (6,), {}),
    "s5_188": (5, (188,), {"calls": 3}),
    "s63_200": (63, (200,), {}),
    "s64_128": (64, (128,), {}),
    "s65_131": (65, (131,), {"calls": 3}),
    "s257_1000": (257, (1000,), {}),
    "s15360_30737": (15360, (30737,), {}),
    "ndim0": (5, (), {}),
    "ndim2": (5, (4, 47), {}),
    "ndim3": (5, (2, 3, 7), {}),
    "symbolic": (5, (4, 47), {"symbolic": True}),
    "zero": (5, (3, 0), {}),
    "edge": (8, (188,), {"edge": True}),
    "inplace": (5, (188,), {"inplace": True}),
}

# name -> (nb_multi, nb_outcomes, n, odtype); each in both pvals dtypes
MULTINOMIAL_CASES = {f"m{nm}_{no}_{n}_{od}": (nm, no, n, od)
                     for nm, no, n, od in ((1, 1, 1, "int64"), (1, 2, 3, "float32"), (1, 65, 1, "auto"),
                                           (1, 1000, 3, "int64"), (65, 1, 3, "auto"), (65, 2, 1, "int64"),
                                           (65, 65, 3, "float32"), (65, 1000, 1, "auto"), (65, 1000, 3, "int64"))}
# name -> (nb_multi, nb_outcomes, n, odtype)
CHOICE_CASES = {f"c{nm}_{no}_{n}": (nm, no, n, od)
                for nm, no, n, od in ((3, 2, 1, "auto"), (3, 2, 2, "auto"), (65, 7, 1, "int64"), (65, 7, 2, "auto"),
                                      (65, 7, 7, "int32"), (5, 65, 1, "auto"), (5, 65, 2, "auto"), (5, 65, 65, "auto"))}


# ---- the generator in plain integers -------------------------------------------------------------
def _wrap(y):
    """The value an int32 holds after a wrapping addition."""
    return (y + (1 << 31)) % (1 << 32) - (1 << 31)


def step(state, hits=None):
    """One step of rng_mrg.py:486-511 on six Python integers: (new state, the integer the sample is
    made of).  ``hits``: a set collecting (correction index, taken) for the six corrections and
    (6, x11 <= x21)."""
    x11, x12, x13, x21, x22, x23 = (int(v) for v in state)

    def correct(k, y, M):
        y = _wrap(y)
        taken = y < 0 or y >= M
        if hits is not None:
            hits.add((k, taken))
        return _wrap(y - M) if taken else y
    y1 = correct(0, ((x12 & 511) << 22) + (x12 >> 9) + ((x13 & 16777215) << 7) + (x13 >> 24), M1)
    y1 = correct(1, y1 + x13, M1)
    x13, x12, x11 = x12, x11, y1
    y1 = correct(2, ((x21 & 65535) << 15) + 21069 * (x21 >> 16), M2)
    y2 = correct(3, ((x23 & 65535) << 15) + 21069 * (x23 >> 16), M2)
    y2 = correct(4, y2 + x23, M2)
    y2 = correct(5, y2 + y1, M2)
    x23, x22, x21 = x22, x21, y2
    if hits is not None:
        hits.add((6, x11 <= x21))
    v = _wrap(x11 - x21 + M1) if x11 <= x21 else _wrap(x11 - x21)
    return [x11, x12, x13, x21, x22, x23], v


def mat_vec(A1k, A2k, state):
    s = [int(v) for v in state]
    return [sum(a * x for a, x in zip(row, s[:3])) % M1 for row in A1k] + \
           [sum(a * x for a, x in zip(row, s[3:])) % M2 for row in A2k]


def substream_states(n_streams, seed=SEED, skip=0):
    """``MRG_RandomStream(seed).get_substream_rstates(n_streams)`` after ``skip`` earlier calls of it
    (each call moves the stream's own state 2^134 steps on): int32 [n_streams, 6]."""
    from aesara_amd.exec_rng import A1, A2, mat_pow_mod
    p72 = (mat_pow_mod(A1, 1 << 72, M1), mat_pow_mod(A2, 1 << 72, M2))
    p134 = (mat_pow_mod(A1, 1 << 134, M1), mat_pow_mod(A2, 1 << 134, M2))
    row = [int(seed)] * 6 if np.ndim(seed) == 0 else [int(v) for v in seed]
    for _ in range(skip):
        row = mat_vec(*p134, row)
    rows = [row]
    for _ in range(1, n_streams):
        rows.append(mat_vec(*p72, rows[-1]))
    return np.asarray(rows, dtype="int32")


def python_dot_modulo():
    """``MRG_RandomStream`` builds its stream states with a small compiled function of its own
    (``multMatVect.dot_modulo``, rng_mrg.py:66).  The C body of that ``DotModulo`` Op does not compile
    against NumPy 2 (``PyArray_Descr.elsize``); its ``perform`` computes the same values, so the
    function is built here with the Python linker before the stream is used.  Needs the reference."""
    import aesara
    from aesara.compile.mode import Mode
    from aesara.sandbox import rng_mrg
    from aesara.tensor.type import iscalar, ivector, lmatrix
    if rng_mrg.multMatVect.dot_modulo is None:
        ins = [lmatrix("A"), ivector("s"), iscalar("m"), lmatrix("A2"), ivector("s2"), iscalar("m2")]
        rng_mrg.multMatVect.dot_modulo = aesara.function(ins, rng_mrg.DotModulo()(*ins), mode=Mode("py", None),
                                                         profile=False)


_STATES = {}


def case_state(name):
    """The input state of a uniform case (a fresh array per call)."""
    n_streams, _, opt = UNIFORM_CASES[name]
    if n_streams not in _STATES:
        _STATES[n_streams] = substream_states(n_streams)
    st = _STATES[n_streams].copy()
    if opt.get("edge"):
        st[:len(EDGE_STATES)] = np.asarray(EDGE_STATES, dtype="int32")
    return st


def sample_file_states():
    """The 12 x 7 states of the reference's ``test_consistency_cpu_serial``: stream i starts 2^134
    steps after stream i-1, its substream j 2^72 steps after substream j-1; int32 [84, 6]."""
    from aesara_amd.exec_rng import A1, A2, mat_pow_mod
    p72 = (mat_pow_mod(A1, 1 << 72, M1), mat_pow_mod(A2, 1 << 72, M2))
    p134 = (mat_pow_mod(A1, 1 << 134, M1), mat_pow_mod(A2, 1 << 134, M2))
    rows, cur = [], [SEED] * 6
    for _ in range(12):
        sub = cur
        for _ in range(7):
            rows.append(sub)
            sub = mat_vec(*p72, sub)
        cur = mat_vec(*p134, cur)
    return np.asarray(rows, dtype="int32")


def load_sample_file():
    return np.loadtxt(os.path.join(MRG_GOLDEN, "samples_MRG31k3p_12_7_5.txt"))


# ---- inputs of the multinomial cases ---------------------------------------------------------------
def _pvals(rng, nm, no, dtype):
    p = rng.random((nm, no)) + 0.05
    return (p / p.sum(axis=1, keepdims=True)).astype(dtype)


def multinomial_inputs(name, pdtype):
    """(pvals, unis, n) of a multinomial case; unis in the dtype of pvals."""
    nm, no, n, _ = MULTINOMIAL_CASES[name]
    rng = np.random.default_rng(1000 + 97 * nm + 13 * no + n)
    return _pvals(rng, nm, no, pdtype), rng.random(nm * n).astype(pdtype), n


def multinomial_special(pdtype, udtype):
    """Rows that sit on the seams: u exactly a partial sum (strict >: the next outcome), u equal to
    the total (a row of zeros), the row [-2, 2, 0] (never above u = 0.5), and an ordinary row; two
    samples each, the second ordinary."""
    p = np.asarray([[0.25, 0.25, 0.5], [0.25, 0.25, 0.25], [-2.0, 2.0, 0.0], [0.5, 0.25, 0.25]], pdtype)
    u = np.asarray([0.25, 0.75, 0.5, 0.6, 0.7, 0.1, 0.5, 0.75], udtype)
    return p, u, 2


def choice_inputs(name, pdtype):
    """(pvals, unis, n) of a choice case.  Uniforms stay below 0.9: after a renormalisation a row
    sums to 1 within a few ulps, so every draw reaches an outcome (the generator asserts it)."""
    nm, no, n, _ = CHOICE_CASES[name]
    rng = np.random.default_rng(2000 + 97 * nm + 13 * no + n)
    return _pvals(rng, nm, no, pdtype), (rng.random(nm * n) * 0.9).astype(pdtype), n


def choice_restated(pvals, unis, n):
    """multinomial.py:344-382 (replace = 0) in NumPy scalars of the C types: (indices, reached)."""
    w = np.array(pvals, copy=True)
    T = w.dtype.type
    nm, no = w.shape
    z = np.zeros((nm, n), "int64")
    reached = np.zeros((nm, n), bool)
    for c in range(n):
        for r in range(nm):
            cummul, u = np.float64(0.0), np.float64(unis[c * nm + r])
            for m in range(no):
                cummul = cummul + np.float64(w[r, m])
                if cummul > u:
                    z[r, c], reached[r, c] = m, True
                    if c == n - 1:
                        break
                    s = T(cummul - np.float64(w[r, m]))
                    w[r, m] = T(0)
                    for k in range(m, no):
                        s = T(s + w[r, k])
                    w[r] = w[r] / s
                    break
    return z, reached


# ---- plans ----------------------------------------------------------------------------------------
def uniform_plan(ndim, dtype, size=None, inplace=False, rstate_dtype="int32", rstate_ndim=2, size_ndim=1):
    """The one-node plan ``mrg_uniform`` lowers to: inputs (rstate[, size]), outputs (new rstate,
    sample); ``size`` an int64 constant, or — ``None`` — a second input."""
    plan = Plan(f"mrg_uniform_{dtype}_{ndim}", {}, [], [], [])
    rstate = plan.new_var(rstate_dtype, [None] * rstate_ndim, "rstate")
    if size is None:
        sz = plan.new_var("int64", [None] * size_ndim, "size")
        plan.inputs = [rstate, sz]
    else:
        sz = plan.add_const(np.asarray(size, "int64").reshape(-1) if size_ndim == 1 else np.asarray(size, "int64"))
        plan.inputs = [rstate]
    new = plan.new_var(rstate_dtype, [None] * rstate_ndim)
    sample = plan.new_var(dtype, [None] * ndim)
    plan.outputs = [new, sample]
    plan.nodes.append(Node("MrgUniform", [rstate, sz], [new, sample],
                           {"inplace": bool(inplace), "ndim": int(ndim), "dtype": dtype}))
    return plan


def op_plan(op, pdtype, udtype, odtype, n=None, pvals_ndim=2, unis_ndim=1):
    """The one-node plan of ``MultinomialFromUniform`` / ``ChoiceFromUniform``: inputs (pvals, unis[,
    n]); ``n`` an int64 scalar constant or — ``None`` — a third input."""
    plan = Plan(f"{op}_{pdtype}_{odtype}", {}, [], [], [])
    pvals = plan.new_var(pdtype, [None] * pvals_ndim, "pvals")
    unis = plan.new_var(udtype, [None] * unis_ndim, "unis")
    if n is None:
        nv = plan.new_var("int64", [], "n")
        plan.inputs = [pvals, unis, nv]
    else:
        nv = plan.add_const(np.asarray(n, "int64"))
        plan.inputs = [pvals, unis]
    out_dt = odtype if odtype != "auto" else (pdtype if op == "MultinomialFromUniform" else "int64")
    out = plan.new_var(out_dt, [None, None])
    plan.outputs = [out]
    plan.nodes.append(Node(op, [pvals, unis, nv], [out], {"odtype": odtype}))
    return plan


def same_lowering(lowered, built):
    """Whether the node of ``lowered`` with the op of ``built``'s only node is that node: same
    parameters, operand dtypes and ranks, output dtypes (an integer operand — ``size``, ``n`` — of any
    width: the front end types a constant ``n`` as int8)."""
    want = built.nodes[0]
    got = [n for n in lowered.nodes if n.op == want.op]
    if len(got) != 1:
        return False

    def sig(plan, vs):
        return [("int" if plan.vars[v].dtype.startswith(("int", "uint")) and plan.vars[v].dtype != "int32"
                 else plan.vars[v].dtype, len(plan.vars[v].shape)) for v in vs]
    return got[0].params == want.params and sig(lowered, got[0].inputs) == sig(built, want.inputs) and \
        sig(lowered, got[0].outputs) == sig(built, want.outputs)


# ---- fixtures -------------------------------------------------------------------------------------
def load_mrg_golden():
    with open(os.path.join(MRG_GOLDEN, "cases.json")) as f:
        return json.load(f)


def _packed_size(a):
    import io
    b = io.BytesIO()
    np.savez_compressed(b, a=a)
    return b.tell()


def save_arrays(name, arrays):
    """One ``<name>.npz``; an array whose compressed size alone exceeds FILE_MAX goes into
    ``<name>__<key>_<i>.npz`` chunks of its flat data.  Returns the paths written."""
    small, paths = {}, []
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= FILE_MAX or _packed_size(a) <= FILE_MAX:
            small[k] = a
            continue
        flat = a.reshape(-1)
        per = FILE_MAX // a.itemsize
        for i in range(0, -(-flat.size // per)):
            p = os.path.join(MRG_GOLDEN, f"{name}__{k}_{i:02d}.npz")
            np.savez_compressed(p, chunk=flat[i * per:(i + 1) * per], shape=np.asarray(a.shape, "int64"))
            paths.append(p)
    p = os.path.join(MRG_GOLDEN, name + ".npz")
    np.savez_compressed(p, **small)
    return paths + [p]


def load_arrays(name):
    with np.load(os.path.join(MRG_GOLDEN, name + ".npz")) as z:
        arrays = {k: z[k] for k in z.files}
    chunks = {}
    for p in sorted(glob.glob(os.path.join(MRG_GOLDEN, f"{name}__*.npz"))):
        key = os.path.basename(p)[len(name) + 2:-len("_00.npz")]
        with np.load(p) as z:
            chunks.setdefault(key, ([], z["shape"]))[0].append(z["chunk"])
    for k, (parts, shape) in chunks.items():
        arrays[k] = np.concatenate(parts).reshape(tuple(int(s) for s in shape))
    return arrays


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(got, want))
