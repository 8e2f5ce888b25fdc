"""Properties of the sym_rare_cases inputs, checked on the CPU: every directed pair sits
where tile_steps evaluates it and has the distance its kind names, and the plain layout
holds nothing the detect-then-fix denominators would flag."""
import numpy as np
import pytest

import sym_rare_cases as R


def test_places_are_distinct_and_in_tile_steps():
    seen = set()
    for kind, a, i, j, _ in R.PLACES:
        assert R.in_tile_steps(R.SIZES[a], i, j), (kind, a, i, j)
        assert (a, i) not in seen and (a, j) not in seen
        seen |= {(a, i), (a, j)}
    # the rule itself: the diagonal tiles and the drain are outside
    assert not R.in_tile_steps(321, 5, 122) and R.in_tile_steps(321, 5, 123)
    assert R.in_tile_steps(321, 63, 320) and not R.in_tile_steps(257, 63, 257)
    assert not R.in_tile_steps(321, 70, 121 + 64) and R.in_tile_steps(321, 70, 122 + 64)
    # both aggregates have a short last tile, and a pair reaches the second's
    assert all(s % 64 == 1 for s in R.SIZES)
    assert any(a == 1 and j == R.SIZES[1] - 1 for _, a, _, j, _ in R.PLACES)
    # one step with two flagged lanes, flagged for different reasons
    steps = {}
    for kind, a, i, j, _ in R.PLACES:
        steps.setdefault((a, i // 64, i + j), set()).add(kind)
    assert any(len(k) >= 2 for k in steps.values())


def test_constants():
    assert all(R.low_word(d) == 0xFFFFFFFF and not R.all_ones(d) for d in R.LOW_ONES)
    assert len({np.frexp(d)[1] for d in R.LOW_ONES}) == len(R.LOW_ONES)  # one per binade
    lo, hi = R.EPS_TRIO[1], R.EPS_TRIO[2]
    assert lo < R.EPS < hi < R.DETECT and np.nextafter(lo, 1.0) == R.EPS == np.nextafter(hi, 0.0)
    assert all(R.all_ones(R.M.HARD_PAIRS[p][0]) for p in R.M.HEAVY_PAIRS)


@pytest.mark.parametrize("dim", R.DIMS)
def test_directed_pairs_have_their_distances(dim):
    case, init, pairs = R.directed(dim)
    assert init.shape == (sum(R.SIZES), dim) and len(pairs) == len(R.PLACES)
    kinds = set()
    for (kind, a, i, j, ci, cj), place in zip(pairs, R.PLACES):
        assert ci == sum(R.SIZES[:a]) + i and cj == sum(R.SIZES[:a]) + j
        assert case["vA"][case["PT"][1][ci]] == a == case["vA"][case["PT"][1][cj]]
        e = init[ci] - init[cj]
        d = float(R.device_distance(init[ci], init[cj]))
        val = place[4]
        if kind == "ones":
            T, e0, e1 = R.M.HARD_PAIRS[val]
            assert d == T and R.all_ones(d)
            if dim >= 2:  # numerators: e0 a power of two
                assert e[0] == e0 and e[1] == e1 and np.frexp(e0)[0] == 0.5
        else:
            assert (e[1:] == 0.0).all() and d == abs(e[0]) == val
            if kind == "eps":
                assert (init[ci][1:] == 0.0).all() and (init[cj][1:] == 0.0).all()
            flagged = not d >= R.DETECT or R.low_word(d) == 0xFFFFFFFF
            assert flagged and not R.all_ones(d)
        kinds.add(kind)
    assert kinds == {"ones", "low-ones", "same", "half-eps", "eps"}
    # the heavy edges are there, both ways
    ip, ix, dx = case["A"]
    for (kind, a, i, j, ci, cj) in pairs:
        if kind == "ones":
            u, v = case["PT"][1][ci], case["PT"][1][cj]
            w = dx[ip[u]:ip[u + 1]][ix[ip[u]:ip[u + 1]] == v]
            assert len(w) == 1 and w[0] in R.M.HEAVY_PAIRS.values()
    # in the shared-reciprocal domain: coordinates 0 or within [2^-200, 2^200]
    assert all(R.M.coord_ok(float(x)) for x in init.reshape(-1))


@pytest.mark.parametrize("dim", [2, 3, 4])  # on a line (d = 1) random members do come close
def test_plain_layout_has_nothing_to_flag(dim):
    _, init = R.plain(dim)
    for a in range(len(R.SIZES)):
        d, norms = R.aggregate_distances(init, a)
        assert d.min() > 2 * R.DETECT and norms.min() > 2 * R.DETECT
        lows = d.view(np.uint64) & np.uint64(0xFFFFFFFF)
        assert not (lows == np.uint64(0xFFFFFFFF)).any()
        assert not ((norms.view(np.uint64) & np.uint64(0xFFFFFFFF)) == np.uint64(0xFFFFFFFF)).any()
