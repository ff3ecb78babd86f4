"""``aesara.map`` over ``det`` / ``matrix_inverse`` / ``eigvalsh`` / ``expm`` of small matrices through the lowering and
the executor's host logic (no GPU): the Scan without recurrence is restated over the whole stack
(scan_rewrite.batch_map_step, ``batched`` nodes) and a dry run makes ONE tile launch for it; above the tile limit the
restated node loops over the single-matrix route; ``eigvalsh(a, b)`` stays a loop."""
import numpy as np
import pytest

import ref_overlay
from test_linalg_lowering import dummy_mode

pytestmark = pytest.mark.skipif(not ref_overlay.available(), reason="reference Aesara not present (GPU box)")

# op -> (the one-launch entry point, the result shape of a step, a launch of the single-matrix route and how often
# three matrices of 65 rows make it: two panels each)
OPS = {"det": ("ahip_lu_tile", lambda n: (), "ahip_lu_det", 3),
       "matrix_inverse": ("ahip_lu_tile", lambda n: (n, n), "ahip_getrf_panel", 6),
       "eigvalsh": ("ahip_syev_tile", lambda n: (n,), "ahip_syev_diag", 3),
       "expm": ("ahip_expm_tile", lambda n: (n, n), "ahip_expm_norm1", 3)}
TILES = {v[0] for v in OPS.values()}


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


def dry_map(ae, fn, *ins):
    """(executor, result, the launches of the executors of restated step plans) of a map of ``fn``."""
    import aesara
    import aesara.tensor as at
    from aesara_amd.executor import PlanExecutor
    syms = [at.dtensor3(f"S{k}") for k in range(len(ins))]
    ys, _ = aesara.map(fn, syms)
    ex = PlanExecutor(ae.function(syms, ys, mode=dummy_mode()).maker.linker.plan, dry_run=True)
    (out,) = ex(*ins)
    rows = [e for k, e in ex._inner.items() if isinstance(k, tuple) and k[0] == "rows" and e]
    return ex, out, [t for e in rows for t in e.trace]


@pytest.mark.parametrize("n", [5, 65])
@pytest.mark.parametrize("op", sorted(OPS))
def test_a_map_over_a_stack_is_restated_over_whole_sequences(ae, op, n):
    """The test that shows the feature: without the map rule the Scan is a ``launch-list`` and the single-matrix
    launches are made three times.  5 rows: exactly one tile launch; 65 rows: the host loop of the restated node."""
    from aesara.tensor import nlinalg, slinalg
    from aesara.tensor.type_other import NoneConst
    fn = {"det": nlinalg.det, "matrix_inverse": nlinalg.matrix_inverse, "expm": slinalg.expm,
          "eigvalsh": lambda a: slinalg.eigvalsh(a, NoneConst)}[op]
    tile, shape, single, count = OPS[op]
    ex, out, trace = dry_map(ae, fn, np.zeros((3, n, n)))
    assert set(ex.scan_modes.values()) == {"all-rows"}, ex.scan_modes
    assert tuple(out.shape) == (3,) + shape(n) and out.dtype == "float64"
    assert all(t.startswith("ahip_") for t in trace), trace
    if n == 5:
        assert [t for t in trace if t in TILES] == [tile] and single not in trace, trace
    else:   # (the blocked eigensolver solves the tiles of its own tournament with ahip_syev_tile)
        assert trace.count(single) == count and (op == "eigvalsh" or tile not in trace), trace


def test_a_map_of_the_generalised_eigenproblem_stays_a_loop(ae):
    from aesara.tensor import slinalg
    from aesara_amd.scan_rewrite import batch_map_step
    ex, out, trace = dry_map(ae, lambda a, b: slinalg.eigvalsh(a, b), np.zeros((3, 5, 5)), np.zeros((3, 5, 5)))
    assert tuple(out.shape) == (3, 5) and not trace
    assert all(m.startswith("launch-list") for m in ex.scan_modes.values()), ex.scan_modes
    scan = next(n for n in ex.plan.nodes if n.op == "Scan")
    assert batch_map_step(scan.params["inner"], scan.params["n_seqs"]) is None
