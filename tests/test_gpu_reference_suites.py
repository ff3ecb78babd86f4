"""The reference's own backend-parameterised test classes under ``mode="HIP"`` on the MI355X
(tests/reference_suites.py: TestBroadcast, TestCAReduce, TestDimShuffle, TestGemm.cmp, TestSgemv /
TestDgemv, TestBlasStrides, the restatement tests of TestScan / TestExamples) — the real
``PlanExecutor``, results converted to ndarrays for the reference's own assertions."""
import pytest

import reference_suites as rs

pytestmark = pytest.mark.gpu


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:                                   # noqa: BLE001
        return False


# the classes need both the reference front end and a device; without them only the test below
# is collected (the same test id everywhere), and it says at run time which one is missing
_BUILT = rs.build(real_device=True) if rs.available() and _has_device() else {}
globals().update(_BUILT)


def test_needs_a_device():
    if not _has_device():
        pytest.skip("no HIP device")
    if not rs.available():
        pytest.skip("no reference front end (oracle/_ref overlay not packed)")
    assert _BUILT, "no reference test class was built under the HIP mode"
