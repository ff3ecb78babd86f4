"""Pin of every generated HIP source: what the generators emit may only change on purpose.

Generated kernels are cached by the hash of their source, so byte-identical sources mean identical
code objects.  For three sets of ``AESARA_HIP_*`` switches this module walks, in a fresh child
process per set (the switches are read at import), what ``prebuild.prebuild_golden_kernels`` walks
— every golden case through ``PlanExecutor(plan, dry_run=True)``, then the full-shape pass — with
``device.compile_cached`` replaced by a recorder of ``sha256(source)``: nothing is compiled.  A few
forms that no dry run selects are generated from hand-built specs, and the forms of the persistent
matrix-state Scan kernel that those shapes miss (``MATRIX_FORMS``) from dry runs at shapes that
select them.  The digests are compared with ``tests/golden/kernel_sources.json``.

A pull request that changes a kernel ON PURPOSE rewrites the fixture with

    python tests/test_kernel_sources.py --update

and says so; a refactor must leave the fixture untouched.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "kernel_sources.json")
FULL_SHAPES = "<full shapes>"

SETS = {
    "default": {},
    "B": {"EW_TRACE": "1", "EARLY": "0", "RED_BLOCKED": "1", "FASTEXP": "0", "FASTDIV": "0",
          "NT": "3", "TILED": "0", "SCAN_PERSIST": "0"},
    "C": {"RED_BLOCKED": "0", "FASTDIV": "1", "UNROLL": "4", "VECBYTES": "16", "HFUSE": "0",
          "GE_WAVES": "8"},
}


def _digest(hashes):
    return hashlib.sha256("\n".join(hashes).encode()).hexdigest()[:16]


def _hand_built():
    """(name, generator, spec) of forms that the dry runs never select."""
    from golden_util import CASES, case_plan

    from aesara_amd import codegen as cg
    from aesara_amd.fusion import build_steps

    def plan_of(name):
        return case_plan(next(c for c in CASES if c["name"] == name))

    sc = plan_of("cfg2_gauss_sum").nodes[3].params["scalar"]
    f64 = ["float64"] * 4
    red = {"kind": "all", "op": "add", "acc": "float64", "out": "float64", "ref": 0}
    flat = dict(idx64=False, reduce=red, block=1024, unroll=2, invariant=[True, False, True, True])
    inner = ["b", "c", "b", "b"]
    yield "flat_all_hjobs", cg.generate, cg.KernelSpec(sc, f64, [], [], inner, 1, 2, hjobs=True, **flat)
    yield "flat_all_hjobs_trace", cg.generate, cg.KernelSpec(sc, f64, [], [], inner, 1, 2, hjobs=True,
                                                             trace=True, **flat)
    yield "flat_all_blocked2_late", cg.generate, cg.KernelSpec(sc, f64, [], [], inner, 1, 2, blocked=2,
                                                               early=False, **flat)
    yield "flat_all_stored_nt_i64", cg.generate, cg.KernelSpec(
        sc, f64, ["float64"], [0], inner + ["c"], 1, 2, idx64=True, reduce=red, block=1024,
        unroll=2, nt=3, invariant=[True, False, True, True], blocked=1, early=True, fast_exp=False)
    yield "tiled_all", cg.generate_tiled, cg.KernelSpec(
        sc, f64, [], [], ["b", "t", "b", "b"], 2, 1, tile_dim=[0, 32], reduce=red,
        invariant=[True, False, True, True])
    yield "tiled_store", cg.generate_tiled, cg.KernelSpec(
        sc, f64, ["float64"], [0], ["b", "t", "b", "b", "c"], 3, 1, tile_dim=[1, 64],
        invariant=[True, False, True, True])

    # the softmax chain, laid out as exec_elemwise._run_rowchain does for one [N, K] operand
    st = next(s for s in build_steps(plan_of("softmax_rows_f32")) if s.kind == "rowchain")
    members, slots = [], 1
    for m in st.extra["members"]:
        sm = {"scalar": m["scalar"], "ins": m["ins"], "reduce": None, "stores": [], "rowlike": False}
        for ref, _ in m["stores"]:
            sm["stores"].append([ref, "float32", slots])
            slots += 1
        if m["reduce"]:
            r = m["reduce"]
            sm["reduce"] = {"op": r["op"], "acc": r["acc"], "ref": r["ref"], "out": "float32",
                            "slot": None}
        members.append(sm)
    ext = [("float32", "f")]
    yield "rowchain", cg.generate_rowchain, cg.RowChainSpec(ext, members, 64, 4, 4)
    yield "rowchain_nt_lead2", cg.generate_rowchain, cg.RowChainSpec(ext, members, 16, 2, 2, lnd=2, nt=True)
    yield "rowchain_long", cg.generate_rowchain_long, cg.RowChainSpec(ext, members, 64, 4, 1, block=512)
    yield "rowchain_long_1024", cg.generate_rowchain_long, cg.RowChainSpec(ext, members, 64, 1, 1, lnd=2,
                                                                         block=1024)


# Forms of the persistent matrix-state Scan kernel (scan_persist_mat) that neither the golden shapes
# nor the full-shape pass select: (name, golden case, (T, B, H), switches, form) — ``form`` is
# (exchange form, batch blocks per workgroup, sequence products in the loop, two operands fetched
# in one polling pass) of a kernel the dry run has to generate (256 CUs in a dry run).
MATRIX_FORMS = [
    ("fwd_b16_h64", "cfg4_gru_b8_f32", (6, 16, 64), {}, ("frag", 1, True, False)),
    ("fwd_b32_h512", "cfg4_gru_b8_f32", (6, 32, 512), {}, ("frag", 1, True, False)),
    # batch slices, sequence products up front, a B = 8 remainder kernel
    ("fwd_b200_h1024_slices", "cfg4_gru_b8_f32", (6, 200, 1024), {}, ("frag", 1, False, False)),
    ("fwd_b32_h512_t2", "cfg4_gru_b8_f32", (2, 32, 512), {}, ("frag", 1, True, False)),
    # gradient Scans with more 16 x 16 tiles than CUs: 2 and 4 interleaved blocks per workgroup
    ("bptt_b128_h1024_nblk2", "gru_bptt_b4_f32", (6, 128, 1024), {}, ("frag", 2, False, True)),
    ("bptt_b256_h1024_nblk4", "gru_bptt_b4_f32", (6, 256, 1024), {}, ("frag", 4, False, True)),
    # ... and a forward Scan that way (h feeds two phases: its blocks run one after the other)
    ("fwd_b128_h1024_nblk2", "cfg4_gru_b8_f32", (6, 128, 1024), {"SM_BATCH_CHUNKS": "0"},
     ("frag", 2, False, False)),
    # float64, four 16-byte fragments per lane and operand
    ("bptt_f64_b16_h128", "gru_bptt_b4_f64", (6, 16, 128), {}, ("frag", 1, False, True)),
    # weights + live fragments beyond 320 registers, blocks fit in LDS: the LDS-image form, and
    # its joint fetch in the gradient Scan
    ("fwd_b16_h1088_lds_image", "cfg4_gru_b8_f32", (6, 16, 1088), {}, ("flag", 1, False, False)),
    ("bptt_b16_h1088_lds_image", "gru_bptt_b4_f32", (6, 16, 1088), {}, ("flag", 1, False, True)),
    ("fwd_b32_h512_trace", "cfg4_gru_b8_f32", (6, 32, 512), {"SM_TRACE": "1"}, ("frag", 1, True, False)),
    ("fwd_b5_h1088_lds_image_trace", "cfg4_gru_b8_f32", (6, 5, 1088), {"SM_TRACE": "1"},
     ("flag", 1, False, False)),
]


def _matrix_forms(data, seen):
    """{name: digest of the sources of the dry run} of MATRIX_FORMS; each run must generate a
    matrix kernel of the form it is listed for."""
    from aesara_amd import knobs
    from aesara_amd import scan_persist_mat as sm
    from aesara_amd.device import DevArray, contiguous_strides
    from aesara_amd.exec_common import _Kernels
    from aesara_amd.executor import PlanExecutor, _FakeBuf
    from aesara_amd.plan import Plan

    def fake(shape, dtype):
        n = 1
        for s in shape:
            n *= s
        return DevArray(_FakeBuf(n, dtype), 0, tuple(shape), contiguous_strides(shape), dtype)

    generated = []
    generate = sm.SpecMat.generate

    def spy(spec):
        joint = any(len(fresh) >= 2 and all(kind == "cur" for _x, kind in fresh)
                    for _e, _l, fresh in sm.phase_fetches(spec.prog))
        generated.append((spec.xmode, spec.nblk, bool(spec.xfold), joint, bool(spec.trace)))
        return generate(spec)

    sm.SpecMat.generate = spy
    got = {}
    try:
        for name, case, (T, B, H), env, form in MATRIX_FORMS:
            plan = Plan.from_json(next(c for c in data if c["name"] == case)["plan"])
            dt = "float64" if case.endswith("f64") else "float32"
            del seen[:], generated[:]
            _Kernels.compiled.clear()
            os.environ.update({"AESARA_HIP_" + k: v for k, v in env.items()})
            try:
                PlanExecutor(plan, dry_run=True)(fake((T, B, H), dt), fake((B, H), dt),
                                                 *[fake((H, H), dt) for _ in range(6)])
            finally:
                for k in env:
                    del os.environ["AESARA_HIP_" + k]
            if int(knobs.get("SCAN_PERSIST")):
                assert form + (bool(env.get("SM_TRACE")),) in generated, (name, generated)
            got[name] = _digest(seen)
    finally:
        sm.SpecMat.generate = generate
    return got


def _collect_here():
    """Body of the child process: the switches of the set are already in the environment."""
    for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from aesara_amd import device

    seen = []

    def record(source):
        seen.append(hashlib.sha256(source.encode()).hexdigest())
        return b""

    device.compile_cached = record          # before anything imports it by name

    from golden_inputs import make_input

    from aesara_amd import prebuild
    from aesara_amd.exec_common import _Kernels
    from aesara_amd.executor import PlanExecutor
    from aesara_amd.plan import Plan

    with open(os.path.join(HERE, "golden", "cases.json")) as f:
        data = json.load(f)["cases"]
    cases, raised, distinct = {}, {}, set()

    def walk(name, fn):
        del seen[:]
        _Kernels.compiled.clear()
        try:
            fn()
        except Exception as e:  # a dry run cannot follow data-dependent control flow
            raised[name] = type(e).__name__
        cases[name] = _digest(seen)
        distinct.update(seen)

    for c in data:
        walk(c["name"], lambda: PlanExecutor(Plan.from_json(c["plan"]), dry_run=True)(
            *[make_input(s) for s in c["inputs"]]))
    import contextlib
    import io
    shown = io.StringIO()
    with contextlib.redirect_stdout(shown):         # it prints the dry runs that raise
        walk(FULL_SHAPES, lambda: prebuild._prebuild_full_shapes({c["name"]: c for c in data}))
    assert "full shape" not in shown.getvalue(), shown.getvalue()
    hand = {}
    for name, gen, spec in _hand_built():
        src, names = gen(spec)
        assert all(n in src for n in names)
        hand[name] = hashlib.sha256(src.encode()).hexdigest()[:16]
    return {"cases": cases, "raised": dict(sorted(raised.items())), "distinct": len(distinct),
            "hand_built": hand, "matrix_forms": _matrix_forms(data, seen)}


def collect(set_name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AESARA_HIP_")}
    env.update({"AESARA_HIP_" + k: v for k, v in SETS[set_name].items()})
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--collect"], env=env, cwd=ROOT,
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    got["env"] = {"AESARA_HIP_" + k: v for k, v in SETS[set_name].items()}
    return got


@pytest.mark.parametrize("set_name", sorted(SETS))
def test_generated_sources_are_pinned(set_name):
    with open(FIXTURE) as f:
        want = json.load(f)[set_name]
    got = collect(set_name)
    assert got["env"] == want["env"]
    for part in ("cases", "hand_built", "matrix_forms"):
        differ = sorted(k for k in set(got[part]) | set(want[part])
                        if got[part].get(k) != want[part].get(k))
        assert not differ, "%s: generated sources changed for %s: %s" % (set_name, part, differ)
    assert got["raised"] == want["raised"]
    assert got["distinct"] == want["distinct"]


if __name__ == "__main__":
    if sys.argv[1:] == ["--collect"]:
        print(json.dumps(_collect_here(), sort_keys=True))
    elif sys.argv[1:] == ["--update"]:
        with open(FIXTURE, "w") as f:
            json.dump({s: collect(s) for s in sorted(SETS)}, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", FIXTURE)
    else:
        sys.exit("usage: test_kernel_sources.py --update")
