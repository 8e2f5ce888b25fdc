"""Aggregate sizes that put the sweeps' record ring (ge_sym.hpp: rec_read / rec_write,
the 16-byte halves, the mirror of slots 0..63 and tile_steps' read one step ahead) at
every edge of its schedule, on random coordinates: every column's record is distinct, so a
read one slot or one half off changes bits.

The sweep of row tile A of an aggregate of `size` members has
ntiles = ceil((size - 64 A) / 64) column tiles; tiles 0 and 1 (the diagonal) and the drain
run col_step, the tiles tt = 2 .. ntiles - 1 run tile_steps (when every record is in the
shared-reciprocal domain).  Even tiles are staged twice (slots 0..63 and their mirror at
128..191), odd tiles once.  tile_steps' 64th step reads ahead into the slot behind its
tile: the next tile's (staged later) or the drain's (zeroed later).
"""
import functools

import numpy as np

import graphs as G
import ref_cases as C

# 257  tile_steps entered once by sweep 2: a one-member last tile directly before the drain
# 320  a full last tile                    321  one member past it
# 384  sweep 0 runs column tiles 2..5: both parities of the mirror twice, a full last tile
# 385  one member past it (tiles 2..6)     448  tiles 2..6 with a full last tile
# 449  a one-member eighth tile after seven full ones
SIZES = [257, 320, 321, 384, 385, 448, 449]
PT_SEED = 7
DIMS = (1, 2, 3, 4)
# REPEL_ONE, the general instantiation, and (2^70: outside weight_ok) the `/` forms, which
# run col_step in every tile: the ring's accessor without tile_steps
REPELS = (1.0, 0.75, 2.0 ** 70)
ITERATIONS = (1, 3)  # the second iteration re-stages a ring that holds the first one's leftovers


def bulk_tiles(size, A):
    """[(tt, members of column tile tt)] of the tiles that sweep A runs in tile_steps."""
    ncols = size - 64 * A
    ntiles = (ncols + 63) // 64
    return [(tt, min(64, ncols - 64 * tt)) for tt in range(2, ntiles)]


def sweeps(size):
    return (size + 63) // 64


@functools.lru_cache(maxsize=None)
def case(dim, repel=1.0, iterations=1, origin_last=False):
    """(case, init): the aggregates of SIZES in one level, a uniform(-1, 1) start in P_T
    storage order.  origin_last: the last member of every aggregate sits at the origin, as
    the padding of a short last tile does, but with the deg+1 the plan builds for it."""
    n = sum(SIZES)
    R = G.rmat(n, 6 * n, seed=13)
    rows = np.repeat(np.arange(n), np.diff(R[0]))
    A = C.symmetric_weights(G.csr_from_edges(n, rows, R[1].astype(np.int64)))
    cs = C._ml(A, SIZES, PT_SEED, dim, iterations, 19, repel=repel)
    init = np.random.RandomState(29 + dim).uniform(-1.0, 1.0, size=(n, dim))
    if origin_last:
        init[np.asarray(cs["PT"][0][1:]) - 1] = 0.0
    init.setflags(write=False)
    return cs, init
