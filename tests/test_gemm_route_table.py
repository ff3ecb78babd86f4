"""The case table of tests/gemm_util.py names every instantiation of aesara_amd/csrc/gemm.hip (no
device needed): deleting a case, or adding an instantiation here without a case, fails."""
import itertools
import re

import gemm_util as gu


def _all_routes(dtype):
    big = ["big/a%d/b%d/e%d" % t for t in itertools.product((0, 1), (0, 1), (0, 1, 2))]
    big += ["big/a%d/b%d/e1" % t for t in ((0, 2), (1, 2), (2, 0), (2, 1), (2, 2))]
    half = ["half/a%d/b%d/e%d/ks%d" % t
            for t in itertools.product((0, 1), (0, 1), (0, 2), (1, 2, 4))]
    # float64 vectors hold two elements: no nf4; four column fragments leave no room for 16 waves
    nfs = (1, 2, 4) if dtype == "float32" else (1, 2)
    skinny = ["skinny/nf%d/bkc%d/nw%d" % (nf, bkc, nw)
              for nf, bkc, nw in itertools.product(nfs, (0, 1), (4, 8, 16)) if not (nf == 4 and nw == 16)]
    assert (len(big), len(half), len(skinny)) == (17, 24, 16 if dtype == "float32" else 12)
    return set(big), set(half + skinny + ["tn", "small", "scale", "none"])


def test_the_table_names_every_instantiation():
    for dtype in gu.DTYPES:
        big, rest = _all_routes(dtype)
        named = {c.route for c in gu.CASES if c.dtype == dtype}
        split = {r for r in named if r.startswith("splitk/")}
        assert named - split == big | rest, (dtype, sorted((named - split) ^ (big | rest)))
        inner = set()
        for r in split:
            m = re.fullmatch(r"splitk/s(2|4|8|16)/(big/.*)", r)
            assert m and m.group(2) in big, r
            inner.add(m.group(2)[-2:])
        assert {"e0", "e2"} <= inner, (dtype, sorted(split))


def test_cases_are_small_and_distinct():
    ids = [c.id for c in gu.CASES]
    assert len(ids) == len(set(ids))
    for c in gu.CASES:
        assert c.dtype in gu.DTYPES and c.family in gu.FAMILIES
        assert 0 <= c.M <= gu.MAX_MN and 0 <= c.N <= gu.MAX_MN and 0 <= c.K <= gu.MAX_K, c.id
        assert 0 <= c.batch <= 3, c.id
        assert set(c.params) <= set(gu.DEFAULTS), c.id


def test_regime_a_sums_are_exact_in_float32():
    """|product| <= 4, K <= 33280, |alpha| <= 2, |beta * Cin| <= 2: every partial sum is a multiple
    of 0.5 below 2**24 / 2, so float32 holds it exactly."""
    assert 2 * (4 * gu.MAX_K) + 2 < 2 ** 23
