#!/usr/bin/env python
"""Generate the MRG31k3p fixtures under tests/golden/mrg/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_pool_golden.py).  Every graph
is built with the reference and evaluated with its C linker (``Mode("cvm", "fast_run")``: the C bodies
are the contract) and, where the two are defined alike, checked against ``Mode("py", ...)`` (the Ops'
``perform``).  tests/golden/mrg/cases.json gets:

* ``matrices``: the reference's ``A1p72`` / ``A2p72`` / ``A1p134`` / ``A2p134`` (what the host power
  routine must reproduce);
* ``uniform``: the cases of mrg_util.UNIFORM_CASES in float32 and float64 — new state and sample of
  every consecutive call (the states, which do not depend on the sample's dtype, in the float32 file); the input states are mrg_util.case_state (held to
  ``get_substream_rstates`` here), the one-node plans mrg_util.uniform_plan (the linker's lowering is
  held to them);
* ``corrections``: how many of the 14 branch outcomes of one step (six corrections and
  ``x11 <= x21``, each both ways) the committed states reach, counted by the plain-integer
  restatement mrg_util.step, which is itself held to every stored sample and state;
* ``multinomial`` / ``choice``: the cases of mrg_util, outputs of the C bodies;
* ``function``: graphs over ``MRG_RandomStream`` (the builders below, which
  tests/test_gpu_mrg_function.py compiles under mode "HIP"): three consecutive draws, a draw after
  ``seed()``, an MLP step with dropout and its gradients, ``normal((1001,))`` with the Box-Muller
  formulas in ``longdouble`` on the same uniforms as ``exact``.

The reference's own data file ``samples_MRG31k3p_12_7_5.txt`` is copied next to them.

Self-checks refuse a case (nothing is written) when C and perform differ where they are defined
alike, when a choice draw reaches no outcome, or when the reference is outside its own bar.

Usage:  python tools/gen_mrg_golden.py
"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_overlay  # noqa: E402

ae = ref_overlay.import_reference()
import aesara.tensor as at  # noqa: E402
from aesara.compile.mode import Mode  # noqa: E402
from aesara.sandbox import multinomial as rmn  # noqa: E402
from aesara.sandbox import rng_mrg  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import mrg_util  # noqa: E402
from conv_util import eps, rel_l2  # noqa: E402
from golden_inputs import make_input  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

mrg_util.python_dot_modulo()
C_MODE = Mode("cvm", "fast_run")
PY_MODE = Mode("py", "fast_run")
FN_SEED, RESEED = 234, 777
N_CALLS = 3


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def lower(ins, outs):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore", accept_inplace=True)
    return f.maker.linker.plan


# ---- op cases ------------------------------------------------------------------------------------
def uniform_graph(ndim, dtype, size=None):
    rstate = at.imatrix("rstate")
    sz = at.lvector("size") if size is None else at.as_tensor_variable(np.asarray(size, "int64").reshape(-1))
    op = rng_mrg.mrg_uniform(TensorType(dtype, shape=(None,) * ndim))
    return [rstate] + ([sz] if size is None else []), list(op(rstate, sz))


def uniform_case(name, dt, hits):
    n_streams, size, opt = mrg_util.UNIFORM_CASES[name]
    sym = bool(opt.get("symbolic"))
    ins, outs = uniform_graph(len(size), dt, None if sym else size)
    plan = lower(ins, outs)
    assert mrg_util.same_lowering(plan, mrg_util.uniform_plan(len(size), dt, None if sym else size)), plan.pretty()
    # (mrg_uniform.perform does not run under NumPy 2 — ``int32 & 0xFFFFFFFF`` raises OverflowError —
    # so the C body is checked against the plain-integer restatement mrg_util.step instead)
    f = ae.function(ins, outs, mode=C_MODE)
    extra = [np.asarray(size, "int64")] if sym else []
    state = mrg_util.case_state(name)
    assert np.array_equal(state[len(mrg_util.EDGE_STATES) if opt.get("edge") else 0:],
                          ref_states(n_streams)[len(mrg_util.EDGE_STATES) if opt.get("edge") else 0:])
    arrays = {}
    for k in range(opt.get("calls", 1)):
        new, sample = (np.array(o) for o in f(state, *extra))
        assert new.dtype == np.int32 and sample.dtype == np.dtype(dt) and sample.shape == tuple(size)
        check_restated(state, new, sample, dt, hits)
        arrays[f"state{k}"], arrays[f"sample{k}"] = new, sample
        state = new
    return arrays


def check_restated(state, new, sample, dt, hits):
    """mrg_util.step reproduces the reference (and collects the branch outcomes it takes)."""
    rows = [list(map(int, r)) for r in state]
    flat = sample.reshape(-1)
    norm = np.float32(4.6566126e-10) if dt == "float32" else np.float64(4.656612873077392578125e-10)
    for i in range(flat.size):
        rows[i % len(rows)], v = mrg_util.step(rows[i % len(rows)], hits)
        want = (np.float32(v) if dt == "float32" else np.float64(v)) * norm
        assert want == flat[i], (i, v, want, flat[i])
    assert np.array_equal(np.asarray(rows, "int32"), new)


_REF_STATES = {}


def ref_states(n_streams):
    if n_streams not in _REF_STATES:
        _REF_STATES[n_streams] = rng_mrg.MRG_RandomStream(mrg_util.SEED).get_substream_rstates(n_streams, "float32")
    return _REF_STATES[n_streams]


def check_jump(hits_unused=None):
    """Jumping k steps by the matrix powers equals stepping k times on the committed kinds of state."""
    from aesara_amd.exec_rng import A1, A2, M1, M2, mat_pow_mod
    rows = [list(r) for r in mrg_util.EDGE_STATES] + [list(map(int, r)) for r in ref_states(5)]
    for row in rows:
        cur = list(row)
        for k in range(1, 40):
            cur, _ = mrg_util.step(cur)
            assert cur == mrg_util.mat_vec(mat_pow_mod(A1, k, M1), mat_pow_mod(A2, k, M2), row), (row, k)


def multi_graph(cls, pdtype, udtype, odtype):
    pvals, unis, n = T(pdtype, 2, "pvals"), T(udtype, 1, "unis"), at.lscalar("n")
    return [pvals, unis, n], [cls(odtype)(pvals, unis, n)]


def multi_case(cls, opname, pvals, unis, n, odtype, py_check):
    pdt, udt = pvals.dtype.name, unis.dtype.name
    ins, outs = multi_graph(cls, pdt, udt, odtype)
    plan = lower(ins, outs)
    assert mrg_util.same_lowering(plan, mrg_util.op_plan(opname, pdt, udt, odtype)), plan.pretty()
    (out,) = ae.function(ins, outs, mode=C_MODE)(pvals, unis, n)
    out = np.array(out)
    if py_check:
        (py,) = ae.function(ins, outs, mode=PY_MODE)(pvals, unis, n)
        assert mrg_util.same_bits(out, np.array(py)), (opname, pdt, odtype)
    return out


# ---- function-level graphs (compiled here with the reference, in the tests under mode "HIP") -------
def fn_uniform(dtype, mode):
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    u = srng.uniform((7, 33), dtype=dtype, nstreams=20)
    return ae.function([], u, mode=mode), srng, []


def fn_dropout(dtype, mode):
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    x = T(dtype, 2, "x")
    y = srng.binomial(size=x.shape, p=0.5, dtype=dtype, nstreams=12) * x
    spec = {"kind": "normal", "seed": 31, "shape": [6, 10], "dtype": dtype, "scale": 1.0, "shift": 0.0}
    return ae.function([x], y, mode=mode), srng, [spec]


def fn_multinomial(dtype, mode):
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    p = T(dtype, 2, "p")
    spec = {"kind": "uniform", "seed": 32, "shape": [9, 5], "dtype": dtype, "low": 0.05, "high": 1.0}
    return ae.function([p], srng.multinomial(pvals=p / p.sum(axis=1, keepdims=True), nstreams=9), mode=mode), srng, [spec]


def fn_choice(dtype, mode):
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    p = T(dtype, 2, "p")
    spec = {"kind": "uniform", "seed": 33, "shape": [9, 5], "dtype": dtype, "low": 0.05, "high": 1.0}
    return ae.function([p], srng.choice(size=2, replace=False, p=p / p.sum(axis=1, keepdims=True), nstreams=9),
                       mode=mode), srng, [spec]


def fn_normal(dtype, mode):
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    return ae.function([], srng.normal((1001,), dtype=dtype, nstreams=30), mode=mode), srng, []


def fn_mlp(dtype, mode):
    """One MLP step with dropout: outputs (loss, dW1, dW2, the mask)."""
    srng = rng_mrg.MRG_RandomStream(FN_SEED)
    x, w1, w2, y = T(dtype, 2, "x"), T(dtype, 2, "w1"), T(dtype, 2, "w2"), at.lvector("y")
    h = at.tanh(at.dot(x, w1))
    mask = srng.binomial(size=h.shape, p=0.5, dtype=dtype, nstreams=16)
    p = at.nnet.softmax(at.dot(h * mask * np.asarray(2.0, dtype), w2))
    loss = at.nnet.categorical_crossentropy(p, y).mean()
    def N(shape, seed, scale):
        return {"kind": "normal", "seed": seed, "shape": list(shape), "dtype": dtype, "scale": scale, "shift": 0.0}
    specs = [N((8, 12), 41, 1.0), N((12, 16), 42, 0.3), N((16, 4), 43, 0.3),
             {"kind": "randint", "seed": 44, "low": 0, "high": 4, "shape": [8], "dtype": "int64"}]
    return ae.function([x, w1, w2, y], [loss] + ae.grad(loss, [w1, w2]) + [mask], mode=mode), srng, specs


FUNCTIONS = {"uniform": fn_uniform, "dropout": fn_dropout, "multinomial": fn_multinomial, "choice": fn_choice}
MLP_K_MAX = 16          # the longest reduction of fn_mlp: the 16 hidden units (and 12 inputs, 8 rows)


def box_muller_exact(u):
    """MRG_RandomStream.normal (rng_mrg.py:1205-1248) on the uniforms ``u`` in longdouble."""
    u = np.asarray(u, np.longdouble)
    h = u.size // 2
    r = np.sqrt(-2 * np.log(u[:h]))
    theta = np.longdouble(2) * np.arctan2(np.longdouble(0), np.longdouble(-1)) * u[h:]
    return np.concatenate([r * np.cos(theta), r * np.sin(theta)])[:1001]


def function_cases():
    cases, files = [], {}
    for dt in mrg_util.DTYPES:
        for name, build in FUNCTIONS.items():
            f, srng, specs = build(dt, C_MODE)
            xs = [make_input(s) for s in specs]
            arrays = {f"draw{k}": np.array(f(*xs)) for k in range(N_CALLS)}
            srng.seed(RESEED)
            arrays["reseeded"] = np.array(f(*xs))
            assert not np.array_equal(arrays["draw0"], arrays["draw1"])
            c = {"name": f"fn_{name}_{dt}", "kind": name, "dtype": dt, "inputs": specs, "calls": N_CALLS}
            cases.append(c)
            files[c["name"]] = arrays
            print(f"[ok] {c['name']}: {N_CALLS} draws and one after seed({RESEED})")
        # normal: exact = Box-Muller in longdouble on the same uniforms
        f, _, _ = fn_normal(dt, C_MODE)
        srng2 = rng_mrg.MRG_RandomStream(FN_SEED)
        u = np.array(ae.function([], srng2.uniform((1002,), dtype=dt, nstreams=30), mode=C_MODE)())
        ref = np.array(f())
        exact = box_muller_exact(u)
        err = rel_l2(ref, exact)
        assert ref.shape == (1001,) and ref.dtype == np.dtype(dt) and 0 < err <= 16 * eps(dt), err
        # (the bar of the test is 4 x this error: the reference itself is inside it by construction)
        cases.append({"name": f"fn_normal_{dt}", "kind": "normal", "dtype": dt, "inputs": [], "ref_err": err})
        hi = exact.astype("float64")          # (longdouble kept as a float64 pair: hi + lo)
        files[f"fn_normal_{dt}"] = {"out": ref, "exact_hi": hi, "exact_lo": (exact - hi).astype("float64"),
                                    "uniforms": u}
        print(f"[ok] fn_normal_{dt}: reference at rel L2 {err:.3e} of the longdouble formulas")
        # MLP step with dropout
        f, _, specs = fn_mlp(dt, C_MODE)
        xs = [make_input(s) for s in specs]
        ref = [np.array(o) for o in f(*xs)]
        c = {"name": f"fn_mlp_{dt}", "kind": "mlp", "dtype": dt, "inputs": specs, "n_out": 4, "K_max": MLP_K_MAX}
        arrays = {f"out{k}": r for k, r in enumerate(ref)}
        if dt == "float32":
            f64, _, _ = fn_mlp("float64", C_MODE)
            exact = [np.array(o) for o in f64(*[x.astype("float64") if x.dtype.kind == "f" else x for x in xs])]
            assert np.array_equal(exact[3], ref[3].astype("float64"))      # the same mask
            c["ref_err"] = [rel_l2(r, e) for r, e in zip(ref, exact)]
            arrays.update({f"exact{k}": e for k, e in enumerate(exact)})
        cases.append(c)
        files[c["name"]] = arrays
        print(f"[ok] {c['name']}: ref_err = {c.get('ref_err')}")
    return cases, files


def main():
    os.makedirs(mrg_util.MRG_GOLDEN, exist_ok=True)
    from aesara_amd.exec_rng import A1, A2, M1, M2, mat_pow_mod
    mats = {k: getattr(rng_mrg, k).tolist() for k in ("A1p72", "A2p72", "A1p134", "A2p134")}
    for k, (A, e, m) in {"A1p72": (A1, 72, M1), "A2p72": (A2, 72, M2), "A1p134": (A1, 134, M1),
                         "A2p134": (A2, 134, M2)}.items():
        assert [list(r) for r in mat_pow_mod(A, 1 << e, m)] == mats[k], k
    check_jump()
    files, hits = {}, set()
    uniform = []
    for name, (n_streams, size, opt) in mrg_util.UNIFORM_CASES.items():
        for dt in mrg_util.DTYPES:
            arrays = uniform_case(name, dt, hits)
            if dt != mrg_util.DTYPES[0]:
                # the state does not depend on the sample's dtype: stored once, with the first dtype
                first = files[f"u_{name}_{mrg_util.DTYPES[0]}"]
                for k in [k for k in arrays if k.startswith("state")]:
                    assert np.array_equal(arrays.pop(k), first[k]), (name, k)
            files[f"u_{name}_{dt}"] = arrays
            uniform.append({"name": f"u_{name}_{dt}", "case": name, "dtype": dt, "calls": opt.get("calls", 1)})
            print(f"[ok] u_{name}_{dt}: {n_streams} streams, size {size}")
    assert len(hits) == 14, sorted(hits)
    # the reference's sample file: 12 streams x 7 substreams x 5 samples, one stream per state row
    src = os.path.join(os.path.dirname(rng_mrg.__file__), "samples_MRG31k3p_12_7_5.txt")
    shutil.copyfile(src, os.path.join(mrg_util.MRG_GOLDEN, "samples_MRG31k3p_12_7_5.txt"))
    ins, outs = uniform_graph(1, "float64", (420,))
    _, s = ae.function(ins, outs, mode=C_MODE)(mrg_util.sample_file_states())
    assert np.array_equal(np.array(s).reshape(5, 84).T.reshape(-1), mrg_util.load_sample_file())
    print("[ok] the sample file is reproduced exactly in float64")
    multinomial, choice = [], []
    for dt in mrg_util.DTYPES:
        for name, (nm, no, n, od) in mrg_util.MULTINOMIAL_CASES.items():
            pvals, unis, n = mrg_util.multinomial_inputs(name, dt)
            out = multi_case(rmn.MultinomialFromUniform, "MultinomialFromUniform", pvals, unis, n, od, True)
            assert out.sum() == nm * n
            files[f"{name}_{dt}"] = {"out": out}
            multinomial.append({"name": f"{name}_{dt}", "case": name, "dtype": dt})
        for udt in mrg_util.DTYPES:
            pvals, unis, n = mrg_util.multinomial_special(dt, udt)
            # (perform raises IndexError on the rows no sum exceeds: the C body is the contract)
            out = multi_case(rmn.MultinomialFromUniform, "MultinomialFromUniform", pvals, unis, n, "int64", False)
            assert out.tolist() == [[0, 1, 1], [1, 0, 0], [0, 0, 0], [0, 1, 1]], out.tolist()
            files[f"mspecial_{dt}_{udt}"] = {"out": out}
            multinomial.append({"name": f"mspecial_{dt}_{udt}", "case": "special", "dtype": dt, "udtype": udt})
        for name, (nm, no, n, od) in mrg_util.CHOICE_CASES.items():
            pvals, unis, n = mrg_util.choice_inputs(name, dt)
            out = multi_case(rmn.ChoiceFromUniform, "ChoiceFromUniform", pvals, unis, n, od, False)
            z, reached = mrg_util.choice_restated(pvals, unis, n)
            assert reached.all(), f"{name}_{dt}: a draw reaches no outcome"
            assert np.array_equal(out, z), (name, dt)
            assert all(len(set(r)) == n for r in out.tolist())          # without replacement
            files[f"{name}_{dt}"] = {"out": out}
            choice.append({"name": f"{name}_{dt}", "case": name, "dtype": dt})
        print(f"[ok] multinomial and choice cases, {dt}")
    fcases, ffiles = function_cases()
    files.update(ffiles)
    n_files = 0
    for name, arrays in files.items():
        for p in mrg_util.save_arrays(name, arrays):
            assert os.path.getsize(p) <= 200_000, (p, os.path.getsize(p))
            n_files += 1
    with open(os.path.join(mrg_util.MRG_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_mrg_golden.py",
                   "ref_mode": "Mode('cvm', 'fast_run'), checked against Mode('py', 'fast_run')",
                   "matrices": mats, "corrections": {"outcomes_hit": len(hits), "of": 14},
                   "uniform": uniform, "multinomial": multinomial, "choice": choice, "function": fcases,
                   "fn_seed": FN_SEED, "reseed": RESEED}, f)
    print(f"{len(files)} cases in {n_files} files written")


if __name__ == "__main__":
    main()
