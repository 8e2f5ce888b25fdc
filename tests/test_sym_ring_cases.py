"""Properties of the sym_ring_cases sizes, checked on the CPU: each size yields the tiles
its comment claims, so the GPU test covers the ring edges it means to."""
import numpy as np

import sym_ring_cases as R


def test_sizes_yield_their_tiles():
    # 257: sweep 2 enters tile_steps once, for one member, directly before the drain
    assert R.bulk_tiles(257, 2) == [(2, 1)] and R.bulk_tiles(257, 3) == []
    assert R.bulk_tiles(257, 0) == [(2, 64), (3, 64), (4, 1)]
    # 320 / 321: a full last tile, and one member past it
    assert R.bulk_tiles(320, 0) == [(2, 64), (3, 64), (4, 64)]
    assert R.bulk_tiles(321, 0) == [(2, 64), (3, 64), (4, 64), (5, 1)]
    # 384: tiles 2..5 (even, odd, even, odd), the last one full; 385: one member past it
    assert R.bulk_tiles(384, 0) == [(tt, 64) for tt in (2, 3, 4, 5)]
    assert R.bulk_tiles(385, 0) == [(tt, 64) for tt in (2, 3, 4, 5)] + [(6, 1)]
    # 448: tiles 2..6 with a full last tile; 449: a one-member eighth tile after seven full
    assert R.bulk_tiles(448, 0) == [(tt, 64) for tt in range(2, 7)]
    assert R.bulk_tiles(449, 0) == [(tt, 64) for tt in range(2, 7)] + [(7, 1)]
    assert R.sweeps(449) == 8 and R.sweeps(448) == 7
    for s in (384, 385, 448, 449):  # both parities of the mirror at least twice
        tts = [tt for tt, _ in R.bulk_tiles(s, 0)]
        assert sum(tt % 2 == 0 for tt in tts) >= 2 and sum(tt % 2 == 1 for tt in tts) >= 2


def test_every_sweep_shape_is_covered():
    # every size is streamed under GE_FAML_RES_CAP=256, and some sweep of every aggregate
    # ends its bulk tiles with a full tile or with a single member
    assert all(s > 256 for s in R.SIZES)
    lasts = {R.bulk_tiles(s, A)[-1][1] for s in R.SIZES for A in range(R.sweeps(s))
             if R.bulk_tiles(s, A)}
    assert lasts == {1, 64}
    # a sweep whose only bulk tile is its last (the look-ahead of its 64th step points at
    # the drain's slots), in both parities of the row tile
    only = {A % 2 for s in R.SIZES for A in range(R.sweeps(s)) if len(R.bulk_tiles(s, A)) == 1}
    assert only == {0, 1}


def test_case_layout():
    cs, init = R.case(3)
    n = sum(R.SIZES)
    assert init.shape == (n, 3) and list(np.diff(cs["PT"][0])) == R.SIZES
    assert len(np.unique(init, axis=0)) == n  # every record distinct
    _, o = R.case(3, origin_last=True)
    ends = np.asarray(cs["PT"][0][1:]) - 1
    assert (o[ends] == 0.0).all() and (np.delete(o, ends, axis=0) == np.delete(init, ends, axis=0)).all()
