/*
 * ge.h -- C ABI of libge.so, the MI355X-native (gfx950) implementation of
 * graph-embed's hot path: multilevel modularity coarsening + ForceAtlas.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.  Every function
 * returns 0 on success or a non-zero GE_ERR_* / HIP error code; the text of the
 * last error on the calling thread is ge_last_error().  (The reference reports
 * errors only through assert; the drop-in headers in graph-embed_amd/include turn a non-zero
 * status into std::runtime_error.)
 *
 * Memory: functions named *_plan_* and ge_fa_plan_step take DEVICE pointers
 * (data resident in HBM); every other entry point takes HOST pointers and moves
 * the data itself.  All device work is enqueued on the context's stream.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to LLNL/graph-embed).
 */
#ifndef GE_H
#define GE_H

#ifdef __cplusplus
extern "C" {
#endif

#define GE_OK 0
#define GE_ERR_ARG 1001     /* invalid argument / shape mismatch */
#define GE_ERR_HIP 1002     /* a HIP runtime call failed */
#define GE_ERR_STATE 1003   /* object used in the wrong state */
#define GE_ERR_NOMEM 1004   /* host allocation failed */
#define GE_ERR_CAPACITY 1005 /* a device-side capacity limit (e.g. the partition's list pool) */

#define GE_MODE_STRICT 0 /* bit-exact with the reference's serial op order */
/* GE_MODE_FAST: re-associated / FMA / rsqrt repulsion, everything else as STRICT.
 * Single level (ge_force_atlas, ge_fa_plan_*): 1e-5 relative bar against STRICT; each
 * repulsion sum is within (n + 16 + 24) 2^-53 sum_j |t_ij| of the exact clamped sum
 * over the n vertices (tests/fa_fast_cases.py), deterministic, and the same bits however
 * the rows are cut into plans.
 * Domain of the closed-form repulsion (single level and multilevel): finite coordinates
 * whose squared differences are finite, i.e. |x_i - x_j|^2 does not overflow
 * (coordinates below ~1.3e154 in magnitude).  Beyond it the pair's reciprocal distance
 * comes out NaN and is taken for a clamped pair (1 / eps), so a pair whose true force
 * is ~0 contributes a huge one; the hot loop carries no instruction for this case.  On
 * the single level a vertex with a NaN or infinite coordinate gives NaN in every
 * component of every sum it takes part in (STRICT: NaN likewise for a NaN coordinate).
 * Multilevel level (ge_force_atlas_ml, ge_faml_plan_*, ge_embed and their *_dist
 * forms), dim <= 4: the streamed aggregates' repulsion runs in closed form
 * (faml_fast_repulse); resident aggregates, member rows, init, centring and radius
 * steps are the STRICT kernels and stay bit-exact.  The bar there is PER ITERATION:
 * each repulsion sum is within (s + 32) 2^-53 sum_j |t_ij| of the exact sum over the
 * s members, and after 1 and 2 iterations the coordinates are within 1e-5 relative
 * (max |dX| / max |X|) of STRICT on well-conditioned levels.  At the embed's horizon
 * (100 iterations) no bar of that kind can hold for any re-association: the
 * reference's own result moves by 1e-5 .. 0.3 (d = 2; 1e-5 .. 2e-2 at d = 3, ~1e-3 at
 * d = 8) when its start is perturbed by 1e-15 .. 1e-12 relative (FAST
 * mode), so FAST and STRICT are there two samples of the same chaotic dynamics.
 * FAST results are deterministic and do not depend on how a plan is cut (whole,
 * subset or shard plans give the same bits). */
#define GE_MODE_FAST 1
/* GE_MODE_FARFIELD: GE_MODE_FAST with a Barnes-Hut style far field for the single
 * level's repulsion (ge_force_atlas, ge_fa_plan_*; graph-embed_amd/csrc/ge_far.hip).
 * What is approximated: every iteration the vertices are sorted along a Morton curve
 * and summarised in a flat hierarchy (leaves of 64 sorted vertices, 16 cells per
 * parent; a cell C has mass M_C = sum (deg_j + 1), centre c_C = sum (deg_j + 1) x_j /
 * M_C and a radius a_C >= max_j |x_j - c_C|).  A work item I (64 or 256 consecutive
 * sorted rows with centre c_I and radius a_I) replaces the members of a cell by one
 * term of mass M_C at c_C when, with Dist = |c_I - c_C|,
 *     a_C <= theta (Dist - a_I)   and   Dist - a_I - a_C >= 1e-5
 * (the second condition: no pair the reference would clamp is ever approximated);
 * otherwise it descends, and a leaf that is not accepted is evaluated pair by pair
 * with FAST's closed-form term.  The decision is made once per item, never per row.
 * The bound, per row i with d_i = (deg_i + 1) repel, A_i the cells accepted for its
 * item, rho = |x_i - c_C|, mu_C = |sum_j m_j (x_j - c_C)|, S_C = sum_j m_j |x_j - c_C|^2
 * and a*_C = max_j |x_j - c_C|:
 *     |F~_i - F_i|_2 <= d_i sum_{C in A_i} [ 2 mu_C / rho^3 + 3 S_C / (rho - a*_C)^4 ]
 *                       + (terms_i + 24) 2^-53 sum |t~|
 * against the exact clamped sum of include/forceatlas.hpp:148-167 (first-order Taylor
 * expansion of x / |x|^3 about x_i - c_C; derivation in tests/test_far_cases.py).
 * Results are deterministic: a row's sum is one lane's chain over cells ascending,
 * children ascending, members ascending.
 * The far field runs when dim <= 4 (not the wide schedule), the plan holds every row
 * (row_begin = 0, row_end = n), every deg_j + 1 is > 0 and n >= far_min (131 072, the
 * measured crossover against FAST at dim 3; GE_FAR_MIN overrides).  In every other case -- row shards and ge_force_atlas_dist,
 * dim >= 5, a non-positive mass, a small level -- and in an iteration whose bounding
 * box is not finite, the plan runs exactly what GE_MODE_FAST runs, with the same bits.
 * theta is ge_fa_params.theta, 0 <= theta < 1.  A single-level iteration of this
 * mode synchronises the stream once (the box check), so its steps cannot be captured
 * into a graph; ge_force_atlas does not capture them.
 *
 * The multilevel level (ge_faml_plan_create, _create_subset, _create_shard, and through
 * them ge_force_atlas_ml, ge_embed, the *_dist forms and the drop-in headers) honours
 * the mode per streamed aggregate.  A streamed aggregate takes the far field when
 * dim <= 4 (not the wide schedule), it has at least far_min_ml members (4096, the measured crossover against FAST at dim 3;
 * GE_FAR_MIN_ML overrides, held to 257 at least), the plan holds it whole (not one of a
 * shard plan's split aggregates) and every internal deg + 1 of the plan's streamed rows
 * is finite and > 0 (checked once at plan creation; a failure sends the whole plan to
 * FAST, reason GE_FAR_MASS).  Everything else -- every other streamed aggregate, all
 * resident aggregates, member rows, init, centring and radius steps -- runs exactly as
 * under GE_MODE_FAST, with FAST's bits; a plan without a far aggregate is a FAST plan.
 * Per far aggregate and iteration the scheme above is applied to its members alone:
 * its own box and scale, Morton keys of GE_FAR_ML_KEY_BITS(dim) bits per axis (41 / 20 /
 * 13 / 10 at dim 1 / 2 / 3 / 4: the aggregate's rank in the plan shares the one sort's
 * key), members ordered by (key, position in P_T storage order), leaves of 64, 16 cells
 * per parent up to a top of at most 16 cells, items of item_rows consecutive sorted
 * rows of one aggregate.  A walk never leaves its aggregate, and the bound above holds
 * per row with the internal degree and the sum of include/forceatlas.hpp:394-410 over
 * the aggregate's members.  ge_faml_plan_run synchronises nowhere: an aggregate whose
 * coordinates are not all finite in an iteration gets all-zero keys (P_T order) and a
 * device flag that rejects every cell, so its rows are one lane's chain over its
 * members in P_T order, GE_MODE_FAST's bits; an aggregate whose members coincide needs
 * nothing special (the 1e-5 gap rejects every cell).  Results are deterministic and the
 * same for whole and subset plans.  A shard plan's split aggregates get FAST's bits, so
 * a split aggregate differs from the same aggregate in a whole plan; sharding one
 * aggregate's far field over ranks is not offered. */
#define GE_MODE_FARFIELD 2

typedef struct ge_ctx ge_ctx;
typedef struct ge_hier ge_hier;
typedef struct ge_csr ge_csr;
typedef struct ge_fa_plan ge_fa_plan;

/* ForceAtlas parameters.  Defaults (ge_fa_params_default) are those of
 * forceAtlas / forceAtlasMultilevel, include/forceatlas.hpp:89-103, :320-331. */
typedef struct ge_fa_params {
  double ks, ksmax, repel, attract, gravity, delta, tolerate;
  int use_weights, linlog, nohubs, normalize;
  unsigned seed; /* mt19937 seed replacing std::random_device (:104-105, :332-333) */
  int mode;      /* GE_MODE_STRICT (default), GE_MODE_FAST or GE_MODE_FARFIELD */
  double theta;  /* GE_MODE_FARFIELD's opening parameter, 0 <= theta < 1 (default 0.5, the
                    conventional Barnes-Hut value); not read in any other mode */
} ge_fa_params;

void ge_fa_params_default(ge_fa_params* p);
const char* ge_last_error(void);
const char* ge_version(void);

/* ---- context: one device + one stream; reentrant, no global mutable state ---- */
int ge_device_count(int* count);
int ge_ctx_create(int device, ge_ctx** out);
int ge_ctx_destroy(ge_ctx* ctx);
/* Enqueue on an external hipStream_t (e.g. torch's current stream); NULL
 * restores the context's own stream. */
int ge_ctx_set_stream(ge_ctx* ctx, void* hip_stream);
int ge_ctx_sync(ge_ctx* ctx);

/* ---- the embedding dimension ----
 * Every device entry point below that takes `dim` -- ge_force_atlas, ge_fa_plan_*,
 * ge_force_atlas_ml, ge_faml_plan_*, ge_embed, ge_radius_step_device and their
 * *_dist / ge_faml_plan_create_shard forms -- accepts 1 <= dim <= 16 (GE_MAX_DIM)
 * with the same bit-exact STRICT contract; anything else is GE_ERR_ARG with a message
 * that names the range.  dim <= 4 has every schedule.  dim >= 5 runs the ordered-pair
 * kernels, the fused per-iteration step (graph replay for long runs) and the
 * one-workgroup kernel in its general form (up to 256 rows): no persistent
 * coarsest-level kernel, no symmetric sweeps, and GE_MODE_FAST runs the STRICT
 * kernels, single level and multilevel alike (exact results satisfy its tolerance;
 * ge_faml_plan_mode then reports GE_MODE_STRICT).
 * GE_WIDE_MIN_DIM=<d> in the environment sends dim >= d (d <= 4) through that
 * schedule too: same results, for comparisons.  ge_embed_via_minimization_ml keeps
 * sending dim > 4 to its host path. */
#define GE_MAX_DIM 16

/* ---- single-level ForceAtlas ----
 * Replaces partition::forceAtlas(A, dim, coords, iterations, ks, ksmax, repel,
 * attract, gravity, useWeights, linlog, nohubs, delta, tolerate, normalize)
 * (include/forceatlas.hpp:89-305) and, with init_random = 1 and
 * iterations = 100000, partition::forceAtlas(A, dim) (:307-312).
 * coords: n*dim row-major, in/out.  init_random != 0 draws U(-1,1) from
 * mt19937(p->seed) in the reference order (:118-125). */
int ge_force_atlas(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                   const double* data, int dim, double* coords, int init_random,
                   int iterations, const ge_fa_params* p);

/* Device-resident ForceAtlas iteration over rows [row_begin, row_end) -- the
 * loop body of include/forceatlas.hpp:146-270 -- for row-sharded multi-GPU use.
 * The plan keeps d_indptr/d_indices/d_data by pointer (caller owns them). */
int ge_fa_plan_create(ge_ctx* ctx, int n, int nnz, const int* d_indptr,
                      const int* d_indices, const double* d_data, int dim,
                      const ge_fa_params* p, int row_begin, int row_end,
                      ge_fa_plan** out);
/* d_x_cur: all n*dim coordinates of this iteration; writes rows
 * [row_begin,row_end) of d_x_next (must not alias d_x_cur). */
int ge_fa_plan_step(ge_fa_plan* plan, const double* d_x_cur, double* d_x_next);
/* The second half of the iteration alone -- attraction in CSR order, gravity,
 * swing and update (include/forceatlas.hpp:169-269) -- with the repulsion sums
 * supplied by the caller (d_frep: (row_end - row_begin)*dim, the value each
 * row's force holds after :151-167).  For measuring the attraction pass at
 * sizes whose all-pairs repulsion is out of reach (configs[4]).  Always runs
 * the CSR row kernels (tiles / heavy segments), also for small levels. */
int ge_fa_plan_attract(ge_fa_plan* plan, const double* d_x_cur, const double* d_frep,
                       double* d_x_next);
/* Kernel timing with HIP events on the plan's stream (0 = off). */
int ge_fa_plan_set_profiling(ge_fa_plan* plan, int enable);
/* Average device ms per launch of the repulsion and attraction/update kernels
 * since profiling was enabled; *launches = steps timed. Synchronises. */
int ge_fa_plan_kernel_ms(ge_fa_plan* plan, double* repulsion_ms, double* attraction_ms,
                         int* launches);
/* One repulsion pass alone (include/forceatlas.hpp:151-167) on the caller's
 * coordinates d_x (n*dim): rows [row_begin, row_end) of the sums go to d_frep
 * ((row_end - row_begin)*dim), what ge_fa_plan_attract takes.  Launches what
 * ge_fa_plan_step launches for the repulsion, in any mode (the fused small-level
 * STRICT step has no separate repulsion: there the ordered-pair kernels run, with the
 * same bits).  The single-level twin of ge_faml_plan_repulse; it synchronises. */
int ge_fa_plan_repulse(ge_fa_plan* plan, const double* d_x, double* d_frep);
/* The forces of the last ge_fa_plan_step or ge_fa_plan_attract -- what the reference's
 * force holds after gravity (include/forceatlas.hpp:205-211), the value the next
 * iteration's swing reads -- copied to d_out ((row_end - row_begin)*dim doubles, device)
 * on the plan's stream; zeros before the first pass.  Read only; it does not
 * synchronise. */
int ge_fa_plan_forces(ge_fa_plan* plan, double* d_out);
/* The classes of the plan's CSR rows (graph-embed_amd/csrc/ge_rows.hpp) and how the last
 * pass finished each heavy row.  classes[6]: tiles, heavy rows, medium rows, light rows,
 * heavy-row segments, segment mode (0 whole rows, 1 binade sums).  heavy_rows and
 * heavy_status (host, classes[1] ints each, either may be NULL; call once with both NULL
 * for the count): the heavy rows' ids in the plan's order (longest first) and, of the
 * last row pass (the attraction pass of ge_fa_plan_step where it runs the row kernels,
 * or ge_fa_plan_attract), one of
 *   GE_ROW_NONE          no row pass has run on the plan;
 *   GE_ROW_BINADE        the segments' integer sums gave the force;
 *   GE_ROW_SERIAL_*      the terms were added in stored order, because (or'ed; every
 *                        test of every dimension is made) FLAG a segment met a tie, a
 *                        term of 2^36 units or more, a non-finite term or a base that is
 *                        not normal; BASE a dimension's repulsion sum is zero, subnormal
 *                        or not finite; RANGE a dimension's prefixes are not known to
 *                        stay strictly inside the base's binade;
 *   GE_ROW_SERIAL_WHOLE  the plan keeps heavy rows whole (segment mode 0): always the
 *                        ordered sum.
 * Diagnostics; the results do not depend on it.  Synchronises. */
#define GE_ROW_NONE 0
#define GE_ROW_BINADE 1
#define GE_ROW_SERIAL_FLAG 2
#define GE_ROW_SERIAL_BASE 4
#define GE_ROW_SERIAL_RANGE 8
#define GE_ROW_SERIAL_WHOLE 16
int ge_fa_plan_rows_info(ge_fa_plan* plan, int* classes, int* heavy_rows, int* heavy_status);
/* GE_MODE_FARFIELD diagnostics.  active: the far field runs; reason: why not
 * (GE_FAR_*).  theta, rows per work item, the levels of the hierarchy (0 = leaves)
 * with each level's cell count and cell size in points (arrays of GE_FAR_MAX_LEVELS).
 * Of the last pass: fallback (1: the bounding box was not finite and the FAST kernels
 * ran; the counters are then zero), cells accepted per level, leaves evaluated pair by
 * pair and pair terms evaluated, each summed over the work items (a few atomics per
 * item), and the device ms of the pass before the item kernel (box, keys, sort,
 * records, summaries) and of the item kernel.  Any output pointer may be NULL.
 * Synchronises. */
#define GE_FAR_MAX_LEVELS 8
#define GE_FAR_ACTIVE 0
#define GE_FAR_NOT_REQUESTED 1 /* mode is not GE_MODE_FARFIELD */
#define GE_FAR_DIM 2           /* dim >= 5 or the wide schedule */
#define GE_FAR_ROW_SHARD 3     /* the plan does not hold every row */
#define GE_FAR_MASS 4          /* some deg + 1 is not > 0 */
#define GE_FAR_SMALL 5         /* n < far_min; multilevel: no streamed aggregate reaches far_min_ml */
#define GE_FAR_ML_KEY_BITS(dim) (41 / (dim)) /* multilevel Morton bits per axis, dim 1..4 */
int ge_fa_plan_far_info(ge_fa_plan* plan, int* active, int* reason, double* theta,
                        int* item_rows, int* levels, int* level_cells, long long* level_points,
                        int* fallback, long long* accepted, long long* exact_leaves,
                        long long* pair_terms, double* prep_ms, double* item_ms);
/* What the last far-field pass used, copied to the host: perm (n: the vertex at each
 * sorted position), keys (n, sorted Morton keys), box (dim + 1: the lower corner and
 * the key scale), cells (per level from the leaves up, level_cells[l] records of
 * dim + 2 doubles {c_0 .. c_{dim-1}, M, a}) and items (ceil(n / item_rows) records of
 * the same form; item q holds the sorted rows [q item_rows, min(n, (q + 1) item_rows))).
 * Any pointer may be NULL.  GE_ERR_STATE unless the far field is active and a pass has
 * run without falling back.  Synchronises. */
int ge_fa_plan_far_layout(ge_fa_plan* plan, int* perm, unsigned long long* keys, double* box,
                          double* cells, double* items);
/* The single-level schedule (graph-embed_amd/csrc/ge_fa_sched.hpp): which kernels a
 * plan's step and repulsion pass launch, and how ge_force_atlas runs its iterations.
 * It changes no result bit.  The GE_* tuning and test knobs of the single level are read
 * from the environment once, when a plan is created or ge_force_atlas is entered, never
 * on a step: a plan keeps its route for its lifetime.
 * ge_fa_sched_query runs the schedule for rows [row_begin, row_end) of n vertices on a
 * device of `cus` compute units with no context or device touched (it reads the
 * environment as ge_fa_plan_create does); masses_ok: what the far field's device check
 * of deg + 1 > 0 would say; nnz and iterations enter the run scalars, which describe
 * ge_force_atlas on the whole level.  out: GE_FA_SCHED_COUNT ints.
 * ge_fa_plan_schedule writes the first GE_FA_SCHED_PLAN_COUNT of them, as the live plan
 * holds them.  The grid scalars hold what their kernel would be launched with on these
 * rows whether or not STEP / REP select it. */
#define GE_FA_STEP_FUSED 0  /* fa_grouped_step: n <= grouped_cap(dim) */
#define GE_FA_STEP_STREAM 1 /* fa_grouped_stream: n <= stream_max */
#define GE_FA_STEP_SPLIT 2  /* the repulsion pass, then the CSR row kernels */
#define GE_FA_REP_GROUPED 0      /* fa_repulse_grouped */
#define GE_FA_REP_ORDERED 1      /* fa_repulse_strict, dim <= 4 */
#define GE_FA_REP_ORDERED_WIDE 2 /* fa_repulse_strict<D, false, 1>, the wide schedule */
#define GE_FA_REP_FAST 3         /* fa_repulse_fast + fa_reduce_parts */
#define GE_FA_REP_SWEEPS 4       /* the symmetric sweeps (ge_sym.hpp) */
#define GE_FA_REP_FARFIELD 5     /* the far field; FAST's kernels when the box is not finite */
#define GE_FA_SCHED_MODE 0  /* effective: wide -> STRICT, a FARFIELD that does not run -> FAST */
#define GE_FA_SCHED_STEP 1  /* ge_fa_plan_step: GE_FA_STEP_* */
#define GE_FA_SCHED_REP 2   /* the split step's repulsion and ge_fa_plan_repulse: GE_FA_REP_* */
#define GE_FA_SCHED_WIDE 3
#define GE_FA_SCHED_LANES 4 /* lanes per row of the fused step / grouped repulsion */
#define GE_FA_SCHED_REPEL_ONE 5 /* the kernels' body flags (wide: 0, the general bodies) */
#define GE_FA_SCHED_LINEAR 6
#define GE_FA_SCHED_PER 7 /* fa_repulse_strict: rows per block, blocks, row slots */
#define GE_FA_SCHED_NB 8
#define GE_FA_SCHED_R 9
#define GE_FA_SCHED_FAST_BLOCKS 10 /* fa_repulse_fast's grid (x, y) */
#define GE_FA_SCHED_FAST_JB 11
#define GE_FA_SCHED_SYM 12 /* the plan holds the sweeps' tables */
#define GE_FA_SCHED_FAR_REASON 13 /* GE_FAR_* */
#define GE_FA_SCHED_FAR_ITEM_ROWS 14
#define GE_FA_SCHED_FPART 15 /* FAST's partial sums are allocated */
#define GE_FA_SCHED_PLAN_COUNT 16
#define GE_FA_SCHED_SMALL 16 /* ge_force_atlas: every iteration in one workgroup */
#define GE_FA_SCHED_SMALL_G_DOMAIN 17  /* its domain-only kernel's lanes per row (0: not run) */
#define GE_FA_SCHED_SMALL_G_GENERAL 18 /* its general kernel's */
#define GE_FA_SCHED_SMALL_STAGED 19    /* the CSR entries are staged in LDS */
#define GE_FA_SCHED_SMALL_HANDOVER 20  /* the iteration the domain-only kernel stops at */
#define GE_FA_SCHED_PERSIST 21   /* the persistent kernel is tried */
#define GE_FA_SCHED_PERSIST_G 22 /* from this many lanes per row down */
#define GE_FA_SCHED_PACKED 23    /* at 64 lanes: the packed rows */
#define GE_FA_SCHED_PACK_ROWS 24 /* 4 or 6 (0: by occupancy) */
#define GE_FA_SCHED_GRAPH 25     /* the per-iteration path replays a captured graph */
#define GE_FA_SCHED_COUNT 26
int ge_fa_sched_query(int n, int row_begin, int row_end, int dim, const ge_fa_params* p, int cus,
                      int nnz, int iterations, int masses_ok, int* out);
int ge_fa_plan_schedule(ge_fa_plan* plan, int* out);
int ge_fa_plan_destroy(ge_fa_plan* plan);

/* ---- many small graphs in one call ----
 * count independent graphs as one block-diagonal CSR: graph g owns rows and
 * columns [off[g], off[g+1]) of N = off[count] vertices.  coords: N*dim in/out.
 * init_random != 0: graph g draws its n_g*dim values from the START of
 * mt19937(seeds ? seeds[g] : p->seed), as a separate ge_force_atlas call would.
 * Contract: for every graph and in every mode the result has the bits of
 * ge_force_atlas on that graph alone with the same parameters and that graph's seed.
 * p->normalize is applied per graph.  The result of a graph does not depend on where
 * it stands in the batch or on what else is in it.  Empty graphs (n_g = 0) and
 * count = 0 are fine.  GE_ERR_ARG, with a message that names the graph: offsets that do
 * not ascend from 0, an entry whose column lies outside its graph's block, and, with no
 * graph to name, dim outside 1..16 and negative iterations.
 * Each graph runs in one of three classes, decided on the host
 * (graph-embed_amd/csrc/ge_fa_sched.hpp, fa_batch_schedule):
 *   GE_FA_BATCH_WAVE    1 <= n_g <= 64 under GE_MODE_STRICT or the wide schedule
 *                       (dim >= 5): one wave per graph, 4 graphs per workgroup, the
 *                       whole class one launch;
 *   GE_FA_BATCH_BLOCK   up to 512 rows (256 on the wide schedule): one workgroup per
 *                       graph, one launch;
 *   GE_FA_BATCH_SERIAL  larger graphs, and every graph under GE_MODE_FAST /
 *                       GE_MODE_FARFIELD at dim <= 4: ge_force_atlas's own device path, one
 *                       graph after another inside the call, after the two launches.
 * ge_fa_batch_sched_query: host only, no device: class and lanes per row (0: serial) of
 * each graph from its rows (sizes) and stored entries, and totals[GE_FA_BATCH_TOTALS] =
 * {waves, blocks, serials, workgroups of the wave launch}.  cls, lanes: count ints each;
 * any of the three may be NULL.  ge_fa_batch_info: the totals of the last
 * ge_force_atlas_batch / ge_embed_via_force_atlas_ml on ctx. */
#define GE_FA_BATCH_WAVE 0
#define GE_FA_BATCH_BLOCK 1
#define GE_FA_BATCH_SERIAL 2
#define GE_FA_BATCH_TOTALS 4
int ge_force_atlas_batch(ge_ctx* ctx, int count, const int* off, const int* indptr,
                         const int* indices, const double* data, int dim, double* coords,
                         int init_random, const unsigned* seeds, int iterations,
                         const ge_fa_params* p);
int ge_fa_batch_sched_query(int count, const int* sizes, const int* entries, int dim,
                            const ge_fa_params* p, int* cls, int* lanes, int* totals);
int ge_fa_batch_info(const ge_ctx* ctx, int* totals);

/* anyToMultilevel(forceAtlas)(A, P_T, v_A, coords_A, r_A, coords, d), src/embed.cpp:23-83
 * over include/forceatlas.hpp:307-312, as one call: per aggregate of P_T the members'
 * internal entries as an r x r matrix (1.0 per stored entry, duplicates summed, self
 * entries kept, rows in P_T order, columns ascending by position in the P_T row), all of
 * them as one ge_force_atlas_batch with init_random on and p->seed for every aggregate,
 * each result divided by its largest norm and placed at coords_A[a] + r_A[a] * (x / max).
 * An aggregate of one member gives what the reference's division gives: its one point,
 * moved off the origin by gravity, lands on the ball's surface, and a layout that ends at
 * the origin divides 0 by 0 (NaN).  The weights of A are not read.  P_T must list every fine vertex once and vertex_A must be
 * its inverse (GE_ERR_ARG otherwise).  totals (may be NULL): as ge_fa_batch_info.
 * iterations: the reference's forceAtlas(A, d) runs 100000. */
int ge_embed_via_force_atlas_ml(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                                int m, const int* pt_indptr, const int* pt_indices,
                                const int* vertex_A, const double* coords_A, const double* r_A,
                                int dim, int iterations, const ge_fa_params* p, double* coords,
                                int* totals);

/* ---- layout energy ----
 * A yardstick for a layout, whatever produced it (graph-embed_amd/csrc/ge_energy.hip;
 * the reference has no such function).  With m_i = deg_i + 1 as the iteration uses it (the
 * weighted row sum under use_weights, else the entry count), d_ij = |x_i - x_j|_2,
 * dh_ij = max(d_ij, 1e-5) (the reference's clamp), a'_ik the attraction weight of a stored
 * entry as include/forceatlas.hpp:180-191 forms it (a = 1 without use_weights; a' = a at
 * delta == 1, 1 at delta == 0, sign(a) |a|^delta otherwise) and psi(d) = d^2 / 2, or
 * (1 + d) log(1 + d) - d under linlog, the five columns of row i are
 *   GE_ENERGY_REP       1/2 repel m_i sum_{j != i} m_j / dh_ij
 *   GE_ENERGY_ATT       1/2 attract sum_{k in row i} a'_ik psi(dh_ik), divided by m_i under
 *                       nohubs (the stored entries as they are, self entries included, as
 *                       the reference's loop takes them)
 *   GE_ENERGY_GRAV      gravity m_i |x_i|_2
 *   GE_ENERGY_PAIRDIST  sum_{j != i} d_ij   (unclamped; 0 for coincident points)
 *   GE_ENERGY_EDGELEN   sum_{k in row i} d_ik   (unclamped, unweighted)
 * and totals[c] is column c summed over the rows asked for.  E = totals[REP] + totals[ATT]
 * + totals[GRAV]; for a symmetric graph with nohubs == 0, -dE/dx_i is the reference's
 * force on i (include/forceatlas.hpp:146-211) wherever no pair is clamped and x_i != 0
 * (tests/test_energy_cases.py checks it by central differences).  With nohubs, or inside
 * the clamp, the reference's force is not a gradient; the values are defined all the
 * same.  The relative edge length
 *   lambda = (totals[EDGELEN] / nnz) / (totals[PAIRDIST] / (n (n - 1)))
 * does not depend on the layout's scale: 1 for a random layout, well below 1 when
 * neighbours are close.  The values ignore ks, ksmax, tolerate, normalize, seed, mode and
 * theta: a plan of any mode, over any row range, and every rank of the sharded form give
 * the same bits.  Every sum has one order: a row's partners in jb = max(1, min(16,
 * ceil(n / 256))) chunks of ceil(n / jb), each chunk a chain over ascending j, the chunks
 * added in order; a row's entries in stored order up to 64 entries, above that 64
 * interleaved chains (entries l, l + 64, ...) added in order l = 0 .. 63; the totals in
 * blocks of 1 024 consecutive rows (zeros past the last): ((v0 + v1) + (v2 + v3)) per
 * four rows, the 256 sums folded in halves (a[t] += a[t + h], h = 128 .. 1), the block
 * sums added in block order.
 * Domain: GE_MODE_FAST's, finite coordinates whose squared differences do not overflow;
 * squared differences that underflow (separations below ~1e-154) read as distance 0.  A
 * vertex with a NaN or infinite coordinate has NaN in its five columns, puts NaN into
 * REP and PAIRDIST of every other row and into ATT and EDGELEN of its neighbours, and so
 * into the totals.
 * The multilevel levels have no such energy (forceAtlasMultilevel's external pull is not
 * conservative, :453-465): the yardstick of an embed is this energy of its output on the
 * level-0 graph. */
#define GE_ENERGY_COLS 5
#define GE_ENERGY_REP 0
#define GE_ENERGY_ATT 1
#define GE_ENERGY_GRAV 2
#define GE_ENERGY_PAIRDIST 3
#define GE_ENERGY_EDGELEN 4
/* d_x: n*dim coordinates (device).  d_rows: (row_end - row_begin)*5 doubles (device,
 * row-major; may be NULL).  totals: 5 doubles (host), over the plan's rows.  Works on a
 * plan of any mode; its buffers are allocated by the first call, and the plan is not
 * disturbed: steps interleaved with energy calls give what they give without them.
 * Synchronises. */
int ge_fa_plan_energy(ge_fa_plan* plan, const double* d_x, double* d_rows, double* totals);
/* The same from host arrays through a temporary plan: coords n*dim, rows n*5 (may be
 * NULL), totals 5.  dim outside 1..16, n < 1, null coords or totals: GE_ERR_ARG. */
int ge_layout_energy(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                     const double* data, int dim, const double* coords, const ge_fa_params* p,
                     double* rows, double* totals);

/* ---- layout neighbours ----
 * The exact k nearest neighbours of a vertex in a layout, and the neighbourhood precision
 * built on them: a second yardstick, which sees what the energy's global sums cannot,
 * whether each vertex still has its own neighbours next to it (graph-embed_amd/csrc/
 * ge_knn.hip, ge_knn.cpp; the reference has no such function).  Brute force over all
 * pairs in fp64, by design: it shares no approximation with any mode.
 *
 * Squared distance.  s_ij has the form of the energy's pair term: e_k = x_i[k] - x_j[k],
 * s = e_0 e_0, then s = fma(e_k, e_k, s) for k = 1 .. d-1.  So s_ij and s_ji have the same
 * bits, and s is +0, positive or not finite.  The run-time-d form (d = 5..16) stores the
 * coordinates past d as +0 on both sides: the extra fma(0, 0, s) return s unchanged and
 * the bits are those of a chain of length d.  No square root and no division are taken.
 *
 * Candidates of a query row i: every j != i (compared by index) whose s_ij is finite.
 * Coincident points are candidates with s = 0.  A pair whose s is NaN or +inf is no
 * candidate in either direction: that covers a NaN or infinite coordinate and squared
 * differences that overflow, and a query row with such a coordinate has no candidates.
 *
 * Neighbours of i: the first min(k, candidates) candidates in ascending order of
 * (s_ij, j); equal s means the lower index first.  idx[q k + t] is the t-th neighbour of
 * query row q and dist2[q k + t] its s; the entries past the last candidate are -1 and
 * +inf.  1 <= k <= GE_KNN_MAX_K.  The order (s, j) is total, so the result is a function
 * of the coordinates alone: it does not depend on the tiling, the j split, the rows asked
 * for or the rank that asks.
 *
 * rows: NULL means every row (n_rows must then be n); otherwise n_rows >= 0 ids in
 * [0, n), in any order, repeats allowed, and the output follows the given order.  The
 * list is how a caller samples rows at a size where n^2 is too much, and how ranks share
 * the work.
 *
 * Neighbourhood precision, for a CSR graph A over the same vertices: g_i = the number of
 * distinct columns j != i stored in row i, k_i = min(g_i, kmax), hits_i = how many of the
 * first k_i neighbours of i are columns of row i.  per_row[2 q + {0, 1}] = {k_i, hits_i}
 * and totals[GE_NBHD_ROWS] = the query rows with k_i > 0, totals[GE_NBHD_K] = sum k_i,
 * totals[GE_NBHD_HITS] = sum hits_i over the query rows (a repeated id counts each time).
 * The precision is the mean of hits_i / k_i over the rows with k_i > 0, or pooled,
 * HITS / K: 1 when every vertex has its graph neighbours nearest, about k / (n - 1) for a
 * random layout.  Rows of A must be ascending (equal neighbours, that is duplicate
 * entries, are fine; A need not be symmetric; its weights are not read). */
#define GE_KNN_MAX_K 64
#define GE_NBHD_TOTALS 3
#define GE_NBHD_ROWS 0
#define GE_NBHD_K 1
#define GE_NBHD_HITS 2
#define GE_KNN_PATH_NONE 0 /* no call on this context yet */
#define GE_KNN_PATH_HOST 1
#define GE_KNN_PATH_DEVICE 2
#define GE_KNN_FORM_NARROW 0 /* d <= 4 at compile time */
#define GE_KNN_FORM_WIDE 1   /* the run-time-d form, d = 5..16 */
/* coords n*dim, rows n_rows ids or NULL, idx n_rows*k, dist2 n_rows*k or NULL; all host.
 * ctx == NULL or GE_KNN_HOST=1 takes the library's host path (the plain double loop, the
 * same bits).  GE_ERR_ARG, with a message that names the range: dim outside 1..16, k
 * outside 1..64, n < 1, n_rows < 0 (or != n without rows), a row id outside [0, n), null
 * coords or idx. */
int ge_layout_knn(ge_ctx* ctx, int n, int dim, const double* coords, int k, int n_rows,
                  const int* rows, int* idx, double* dist2);
/* The same on device pointers: enqueues on the context's stream and does not
 * synchronise.  Needs a context; its scratch belongs to the context and is made by the
 * first call (a later call that needs more reallocates it).  The ids of d_rows cannot be
 * checked without waiting: an id outside [0, n) reads nothing and gets no neighbours. */
int ge_layout_knn_device(ge_ctx* ctx, int n, int dim, const double* d_x, int k, int n_rows,
                         const int* d_rows, int* d_idx, double* d_dist2);
/* per_row n_rows*2 ints or NULL, totals GE_NBHD_TOTALS.  The neighbours come from
 * ge_layout_knn with k = kmax (same paths, same errors; kmax outside 1..64 is
 * GE_ERR_ARG); a row of A that is not ascending, a bad indptr or a column outside [0, n)
 * is GE_ERR_ARG with a message that names the row. */
int ge_layout_neighbourhood(ge_ctx* ctx, int n, const int* indptr, const int* indices, int dim,
                            const double* coords, int kmax, int n_rows, const int* rows,
                            int* per_row, long long* totals);
/* The last call on ctx (diagnostics; no result depends on it): the path (GE_KNN_PATH_*),
 * the kernel form (GE_KNN_FORM_*), the query rows per workgroup (256, 128 or 64: the most
 * whose lists of k entries of 12 bytes fit beside the partner tile in half a CU's LDS; 0
 * on the host path), the j splits (each a chain over ascending j whose sorted partial
 * lists a second kernel merges under the full order; GE_KNN_JSPLIT = 1..16 forces the
 * number, read once per call) and the list insertions summed over the call's chains,
 * counted on the device with one atomic per wave.  Read it once the call's work is
 * complete: after a host-pointer call returns, or after ge_ctx_sync following
 * ge_layout_knn_device.  Any pointer may be NULL. */
int ge_knn_info(const ge_ctx* ctx, int* path, int* form, int* rows_per_wg, int* jsplit,
                long long* insertions);

/* ---- multilevel ForceAtlas ----
 * Replaces partition::forceAtlasMultilevel(A, P, v_A, coords_A, r_A, coords,
 * dim, iterations, ks, ksmax, useWeights, linlog, nohubs, repel, attract,
 * gravity, delta, tolerate) (include/forceatlas.hpp:314-574), in the reference's
 * single-thread random draw order.  m = P_T rows; coords: n*dim out. */
int ge_force_atlas_ml(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                      const double* data, int m, const int* pt_indptr,
                      const int* pt_indices, const int* vertex_A, const double* coords_A,
                      const double* r_A, double* coords, int dim, int iterations,
                      const ge_fa_params* p);

/* Device-resident multilevel level (the bench and multi-GPU path).  Aggregates
 * [agg_begin, agg_end) of P_T are processed; h_pt_indptr is a HOST copy of
 * P_T's indptr (used to bucket aggregates by size), every other array is on the
 * device.  Run: d_init = the n*dim draws in P_T storage order (ge_uniform_stream),
 * d_coords receives the members' coordinates (fine-vertex order). */
typedef struct ge_faml_plan ge_faml_plan;
int ge_faml_plan_create(ge_ctx* ctx, int n, const int* d_indptr, const int* d_indices,
                        const double* d_data, int m, const int* h_pt_indptr,
                        const int* d_pt_indptr, const int* d_pt_indices, const int* d_vertex_A,
                        int dim, const ge_fa_params* p, int iterations, int agg_begin,
                        int agg_end, ge_faml_plan** out);
/* The same for an arbitrary set of aggregates (h_aggs: n_aggs strictly increasing
 * ids) -- one rank's share when aggregates are dealt to GPUs by cost
 * (ge_amd.dist.assign_aggregates). */
int ge_faml_plan_create_subset(ge_ctx* ctx, int n, const int* d_indptr, const int* d_indices,
                               const double* d_data, int m, const int* h_pt_indptr,
                               const int* d_pt_indptr, const int* d_pt_indices,
                               const int* d_vertex_A, int dim, const ge_fa_params* p,
                               int iterations, const int* h_aggs, int n_aggs,
                               ge_faml_plan** out);
/* One rank's plan when aggregates are also split across GPUs (SURVEY.md 8(e);
 * include/forceatlas.hpp:394-410 is a per-row ordered sum, so rows of one aggregate
 * can live on different ranks): h_aggs are this rank's whole aggregates, h_split the
 * aggregates split by 64-row tiles over all ranks of comm (the same list on every
 * rank; rank r takes tiles [T r / N, T (r + 1) / N)).  The split aggregates' rows are
 * all-gathered over comm after every iteration inside ge_faml_plan_run, and every
 * rank ends with all their members' coordinates.  Every rank must run its plan. */
typedef struct ge_comm ge_comm;
int ge_faml_plan_create_shard(ge_ctx* ctx, ge_comm* comm, int n, const int* d_indptr,
                              const int* d_indices, const double* d_data, int m,
                              const int* h_pt_indptr, const int* d_pt_indptr,
                              const int* d_pt_indices, const int* d_vertex_A, int dim,
                              const ge_fa_params* p, int iterations, const int* h_aggs,
                              int n_aggs, const int* h_split, int n_split, ge_faml_plan** out);
int ge_faml_plan_run(ge_faml_plan* plan, const double* d_coords_A, const double* d_r_A,
                     const double* d_init, double* d_coords);
/* The mode the plan runs: GE_MODE_FARFIELD when at least one aggregate runs the far
 * field; else GE_MODE_FAST only when faml_fast_repulse is scheduled (the caller asked
 * for FAST or FARFIELD, the plan has streamed rows and dim is not on the wide
 * schedule); otherwise GE_MODE_STRICT.  fast_items: the row items of one
 * faml_fast_repulse launch (under FARFIELD: those that remain).  Under FAST and
 * FARFIELD the STRICT schedule knobs (GE_FAML_SYM*, GE_FAML_R / U) are ignored and
 * ge_faml_plan_schedule reports zeros. */
int ge_faml_plan_mode(ge_faml_plan* plan, int* mode, int* fast_items);
/* One repulsion pass of the plan's streamed aggregates alone (include/forceatlas.hpp:
 * 394-410) on the caller's coordinates d_x (n*dim, P_T storage order): each streamed
 * row's sum is written to d_frep in the same layout, positions of other members are
 * left untouched.  Launches what ge_faml_plan_run launches per iteration, in either
 * mode.  A measurement and test hook like ge_fa_plan_attract; it synchronises and
 * does not disturb later runs. */
int ge_faml_plan_repulse(ge_faml_plan* plan, const double* d_x, double* d_frep);
/* GE_MODE_FARFIELD diagnostics of a multilevel plan.  active: at least one aggregate
 * runs the far field; reason: why not (GE_FAR_*).  theta, far_min_ml, rows per item,
 * Morton key bits per axis, the far aggregates and their rows.  Of the last pass
 * (ge_faml_plan_repulse, or the last iteration of a run): the aggregates whose box was
 * not finite, cells accepted per level (GE_FAR_MAX_LEVELS), leaves evaluated pair by
 * pair, pair terms, and the device ms of the pass before the item kernel and of the
 * item kernel.  Any output pointer may be NULL.  Synchronises; results do not depend
 * on it. */
int ge_faml_plan_far_info(ge_faml_plan* plan, int* active, int* reason, double* theta,
                          int* far_min_ml, int* item_rows, int* key_bits, int* aggregates,
                          long long* rows, int* bad_boxes, long long* accepted,
                          long long* exact_leaves, long long* pair_terms, double* prep_ms,
                          double* item_ms);
/* The plan's far aggregates (ge_faml_plan_far_info's count), larger first, and the
 * sizes of one's layout: members, levels, cells per level from the leaves up
 * (GE_FAR_MAX_LEVELS ints) and items.  GE_ERR_ARG if agg is not a far aggregate. */
int ge_faml_plan_far_aggregates(ge_faml_plan* plan, int* aggs);
int ge_faml_plan_far_shape(ge_faml_plan* plan, int agg, int* members, int* levels,
                           int* level_cells, int* items);
/* What the last pass used for far aggregate agg, in ge_fa_plan_far_layout's record
 * form: perm (the position within the aggregate at each sorted position), keys (the
 * sorted Morton keys), box (dim + 1), cells per level from the leaves up and items.
 * GE_ERR_ARG if agg is not a far aggregate of the plan, GE_ERR_STATE before a pass.
 * Any pointer may be NULL.  Synchronises. */
int ge_faml_plan_far_layout(ge_faml_plan* plan, int agg, int* perm, unsigned long long* keys,
                            double* box, double* cells, double* items);
int ge_faml_plan_set_profiling(ge_faml_plan* plan, int enable);
/* Average device ms of the resident (LDS) kernels and of the streamed path per run
 * (under GE_MODE_FARFIELD the far passes are part of the streamed path). */
int ge_faml_plan_kernel_ms(ge_faml_plan* plan, double* resident_ms, double* streamed_ms,
                           int* runs);
/* Average device ms of one streamed-path repulsion launch (the sweeps, faml_big_repulse
 * or, under GE_MODE_FAST, faml_fast_repulse, under GE_MODE_FARFIELD the far pass and it; one per iteration) over the profiled runs, and the ordered pairs one launch
 * evaluates (sum of s(s-1) over the streamed aggregates); 0 launches if none. */
int ge_faml_plan_repulse_ms(ge_faml_plan* plan, double* ms_per_launch, int* launches,
                            double* pairs_per_launch);
/* Average device ms of one pass over the streamed members' rows (FamlRows: CSR
 * attraction / external pull, :415-467, gravity and update, :469-530; one per
 * iteration), the passes profiled, and the rows and CSR entries one pass reads. */
int ge_faml_plan_rows_ms(ge_faml_plan* plan, double* ms_per_pass, int* passes,
                         long long* rows, long long* entries);
/* The plan's schedule of the streamed aggregates' repulsion: how many run as
 * plain symmetric sweeps, in bands (pre row blocks / in-band sweeps / post row
 * blocks: a shorter dependency chain), as whole row blocks, and the units of
 * one launch.  Diagnostics; the results do not depend on it. */
int ge_faml_plan_schedule(ge_faml_plan* plan, int* sweeps, int* banded, int* row_blocks,
                          int* units);
/* The size class every aggregate of the plan took and the kernels that run them.
 * res_cap: the largest aggregate kept resident in LDS (GE_FAML_RES_CAP overrides the
 * plan's rule; clamped to [256, the large kernel's capacity at this dim]).
 * aggregates[4]: small (<= 64 members), mid (<= 256), large-resident (<= res_cap),
 * streamed (a shard plan's split aggregates included).  blocks[3]: blocks of the
 * small, mid and large resident launches.  rows[6]: the classes of the streamed
 * members' CSR rows -- tiles, heavy rows, heavy-row segments, segment mode (0 whole
 * rows, 1 binade sums, 2 stored terms), early heavy rows (the late ones are
 * heavy - early), the early rows' segments.  Diagnostics; the results do not
 * depend on it. */
int ge_faml_plan_classes(ge_faml_plan* plan, int* res_cap, int* aggregates, int* blocks,
                         int* rows);
int ge_faml_plan_destroy(ge_faml_plan* plan);
/* The schedule a plan would settle on, computed on the host alone (no device is
 * touched): what ge_faml_plan_create* builds from P_T's indptr, the aggregate lists
 * (h_split: the aggregates split over nranks ranks, as ge_faml_plan_create_shard),
 * the dimension, ge_fa_params.mode and the GE_FAML_* environment, given the device's
 * CU count and the blocks per CU of the symmetric sweep kernel (sym_occ).  Tables are
 * int arrays owned by the handle: the resident packs' aggregates and their block
 * offsets (small, mid, large), this rank's streamed rows, the rows it initialises,
 * the aggregates centred at the end, the split rows by rank and their counts, the
 * STRICT items (2 ints each), the FAST items and the sweep units (4 ints each), and
 * the scalars {res_cap, aggregates[4], mid and large offsets into the block table,
 * blocks[3], R, U, variant code, fast, sym, wide, progress tiles, sweeps, row blocks,
 * sym blocks}.  Diagnostics and tests; the results do not depend on the schedule. */
typedef struct ge_faml_sched ge_faml_sched;
#define GE_FAML_SCHED_ORDER 0
#define GE_FAML_SCHED_BEG 1
#define GE_FAML_SCHED_ROWS 2
#define GE_FAML_SCHED_IROWS 3
#define GE_FAML_SCHED_HUGE 4
#define GE_FAML_SCHED_XROWS 5
#define GE_FAML_SCHED_XCOUNTS 6
#define GE_FAML_SCHED_ITEMS 7
#define GE_FAML_SCHED_FITEMS 8
#define GE_FAML_SCHED_UNITS 9
#define GE_FAML_SCHED_SCALARS 10
/* mode = GE_MODE_FARFIELD: the aggregates that take the far field, larger first (they
 * are then no FAST items); GE_FAR_MIN_ML is read from the environment like GE_FAML_*. */
#define GE_FAML_SCHED_FARAGGS 11
int ge_faml_sched_create(int m, const int* h_pt_indptr, const int* h_aggs, int n_aggs,
                         const int* h_split, int n_split, int rank, int nranks, int dim,
                         int mode, int cus, int sym_occ, ge_faml_sched** out);
int ge_faml_sched_table(const ge_faml_sched* sched, int k, const int** data, long long* len);
/* Ordered pairs one repulsion launch of the streamed rows evaluates. */
int ge_faml_sched_pairs(const ge_faml_sched* sched, double* streamed_pairs);
int ge_faml_sched_destroy(ge_faml_sched* sched);

/* ---- coarsening hierarchy ----
 * Replaces std::vector<SparseMatrix> partition::partition(A, coarseningFactor,
 * printing, positiveMerging, stallStopThreshold, matchingIterations,
 * mergeLeaves) (include/partitioner.hpp:52-53, src/partitioner.cpp:1550-1893).
 * A must be symmetric.  Level l of the result is P_T[l] (rows x cols, one 1.0
 * per column).  ctx != NULL builds the hierarchy on the context's device
 * (graph-embed_amd/csrc/ge_partition_dev.hip) when A is symmetric with equal
 * mirror weights, strictly ascending rows and finite weights none of which is
 * -0.0: integer weights (|w| <= 2^40, sum |w| < 2^52) by the exact contraction,
 * any other real weights by the ordered contraction, which adds in the
 * reference's order.  ctx == NULL, other inputs, or GE_PARTITION_HOST=1 take the
 * host path.  All give the reference's P_T arrays and its final weights, bit
 * for bit.  merge_leaves != 0 is rejected. */
int ge_partition(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                 const double* data, double coarsening_factor, int printing,
                 int positive_merging, double stall_stop_threshold,
                 int matching_iterations, int merge_leaves, ge_hier** out);
/* Replaces the one-level overloads SparseMatrix partition::partition(A, printing,
 * ...) (src/partitioner.cpp:970-1266; num_parts <= 0) and partition(A, numParts,
 * printing, ...) (:1272-1544): the same rounds without snapshots, stopped by the
 * stall test or once at most num_parts aggregates are left.  The result has
 * exactly one level, P_T over all n columns.  Same paths as ge_partition. */
int ge_partition_single(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                        const double* data, int num_parts, int printing,
                        int positive_merging, double stall_stop_threshold,
                        int matching_iterations, int merge_leaves, ge_hier** out);
/* Which path built h, its rounds, and the lists rebuilt over all rounds by the
 * device's wave, block and global kernels (zero on the host path).  Any output
 * pointer may be NULL. */
#define GE_PARTITION_PATH_HOST 0
#define GE_PARTITION_PATH_DEVICE_EXACT 1
#define GE_PARTITION_PATH_DEVICE_ORDERED 2
int ge_hier_info(const ge_hier* h, int* path, int* rounds, long long rebuilt[3]);
/* Which kernel class of the device partition handled what, for tests.  Collected
 * only when GE_PARTITION_CENSUS=1 is set when ge_partition / ge_partition_single
 * is called (device counters carried out with each round's export: no extra
 * synchronisation, copy or output); all zeros otherwise and on the host path.
 * Every field is a sum over rounds and passes except match_max_candidates; the
 * 32-bit device counters are folded into these 64-bit sums at every round's
 * export, so a sum is exact while one round adds less than 2^32 to it. */
typedef struct ge_partition_census {
  /* lists scanned: one thread (<= 16 entries), one wave (<= 512), one block
   * (<= 16 384), 64 chunk blocks and a combining wave (longer) */
  long long scan_small, scan_mid, scan_big, scan_huge;
  /* vertices that kept a result without a rescan: pass 0 by the bound recorded at
   * the last pass-0 scan, pass >= 1 by the recorded runner-up, last pass by the
   * recorded bound being non-positive */
  long long kept_bound, kept_runner_up, kept_nonpositive;
  /* rescans of lists longer than 16 entries by reason: list or alpha changed, the
   * recorded bound failed, the argmax was touched */
  long long rescan_changed, rescan_bound, rescan_touched;
  /* the matching's last kernel: locally-dominant rounds on global memory (more
   * than 1 024 live candidates) and in LDS; the largest candidate count it received */
  long long match_global_rounds, match_lds_rounds, match_max_candidates;
  /* lists rebuilt per table class (as ge_hier_info), written back in place or
   * moved to fresh pool space */
  long long rebuilt_wave, rebuilt_block, rebuilt_global;
  long long rebuilt_in_place, rebuilt_moved;
  /* hub lists (longer than 2 048) patched in place; global-class lists rebuilt
   * instead because the list is short, a set is too small (more than 1 024
   * absorbed neighbours or partner entries) or the result does not fit */
  long long patched, patch_short, patch_size, patch_fit;
  /* rounds whose merges exceeded the 4 096 records exported with the counts;
   * compactions of the list pool and of the alive list */
  long long record_refetches, pool_compactions, alive_compactions;
} ge_partition_census;
int ge_hier_census(const ge_hier* h, ge_partition_census* out);
/* What the round loop ended with: the adjacency a[i][k] of the vertices alive at
 * loop exit (rows and columns numbered by `used` slot = the last P_T's row
 * number, columns ascending; free with ge_csr_free) and their alpha (one per row
 * of the last P_T). */
int ge_hier_final_graph(const ge_hier* h, ge_csr** adj);
int ge_hier_final_alpha(const ge_hier* h, double* alpha);
int ge_hier_levels(const ge_hier* h, int* levels);
int ge_hier_shape(const ge_hier* h, int level, int* rows, int* cols);
/* indptr: rows+1 ints, indices: cols ints */
int ge_hier_copy(const ge_hier* h, int level, int* indptr, int* indices);
int ge_hier_free(ge_hier* h);

/* Replaces partition::interpolationMatrix(numCols, partition)
 * (src/partitioner.cpp:29-65) in flattened form: sets[offsets[r]..offsets[r+1])
 * are row r's columns. */
int ge_interpolation_matrix(int num_cols, int num_rows, const int* offsets,
                            const int* sets, ge_csr** out);

/* ---- P^T A P on the device ----
 * Replaces P_T.Mult(A).Mult(P_T.Transpose()) (examples/embed.cpp:96-98,
 * examples/embedder.cpp:213-216; linalgcpp).  Output rows sorted ascending. */
int ge_ptap(ge_ctx* ctx, int n, const int* indptr, const int* indices, const double* data,
            int m, const int* pt_indptr, const int* pt_indices, ge_csr** out);
/* Coarse rows [a0, a1) of the same product, 0 <= a0 <= a1 <= m: a1 - a0 rows of m
 * columns (the row-range form that ge_ptap_dist gives each rank its share with). */
int ge_ptap_rows(ge_ctx* ctx, int n, const int* indptr, const int* indices, const double* data,
                 int m, const int* pt_indptr, const int* pt_indices, int a0, int a1,
                 ge_csr** out);
/* What the last P^T A P call on ctx did (ge_ptap, ge_ptap_rows, a rank's share of
 * ge_ptap_dist): the key widths in bits of j (bn), of the column aggregate (bb) and
 * of the row (ba), which sort ran, the emitted entries and the (row, column) runs.
 * GE_PTAP_SORT_NONE: the call returned before sorting (nothing to emit). */
enum {
  GE_PTAP_SORT_NONE = 0,
  GE_PTAP_SORT_SINGLE = 1,         /* one sort of the composite key, <= 64 bits */
  GE_PTAP_SORT_SPLIT_WIDTH = 2,    /* split sort: the key needs more than 64 bits */
  GE_PTAP_SORT_SPLIT_OVERRIDE = 3  /* split sort by GE_PTAP_SPLIT_SORT alone */
};
int ge_ptap_info(const ge_ctx* ctx, int* bn, int* bb, int* ba, int* sort, long long* entries,
                 long long* runs);
int ge_csr_shape(const ge_csr* c, int* rows, int* cols, long long* nnz);
int ge_csr_copy(const ge_csr* c, int* indptr, int* indices, double* data);
int ge_csr_free(ge_csr* c);

/* ---- modularity (src/partitioner.cpp:69-114) ---- */
int ge_modularity(int n, const int* indptr, const int* indices, const double* data,
                  int m, const int* vertex_A, double* q);
/* The same with the CSR and vertex_A on the device (O(nnz) pass as 64-bit integer
 * sums -- exact, the weights being truncated to int -- then the O(M) final sum on
 * the host in the reference's order).  Same result bits as ge_modularity. */
int ge_modularity_device(ge_ctx* ctx, int n, const int* d_indptr, const int* d_indices,
                         const double* d_data, int m, const int* d_vertex_A, double* q);

/* ---- multilevel embed ----
 * Replaces partition::embed(As, P_Ts, d) (include/embed.hpp:70-72,
 * src/embed.cpp:561-796).  levels = P_Ts.size(); As has levels+1 entries.
 * a_* are the concatenated CSR arrays of As[0..levels], p_* of
 * P_Ts[0..levels-1]; a_n[l] = rows of As[l]; *_off / *_nz_off = start of each
 * level in the indptr / indices arrays.  base_iterations / ml_iterations:
 * reference values 100000 and 100.  print_progress mirrors the reference's
 * "embedding layer" stdout lines (:583, :613). */
int ge_embed(ge_ctx* ctx, int levels, const int* a_n, const int* a_off,
             const int* a_nz_off, const int* a_indptr, const int* a_indices,
             const double* a_data, const int* p_rows, const int* p_off,
             const int* p_nz_off, const int* p_indptr, const int* p_indices, int dim,
             int base_iterations, int ml_iterations, int print_progress,
             const ge_fa_params* p, double* coords_out);

/* Radius ("kinetic ball") step between levels, src/embed.cpp:615-777 (host).
 * m coarse vertices with coords_A (m*dim, updated in place by the rescale of
 * :757-777 unless coarse_is_base) -> r_A (m).  coarse_is_base selects the
 * all-pairs base case (:616-679); otherwise P_T[l+1] (mc rows), coords_Ac /
 * r_Ac of level l+2 and A_c = As[l+1] (ac_indptr/ac_indices) are used. */
int ge_radius_step(int m, double* coords_A, double* r_A, int dim, int coarse_is_base, int mc,
                   const int* ptc_indptr, const int* ptc_indices, const double* coords_Ac,
                   const double* r_Ac, const int* ac_indptr, const int* ac_indices);

/* The same step on the device (graph-embed_amd/csrc/ge_radius.hip): the events
 * pop in parallel rounds with the serial loop's result bits.  When an event
 * distance is 0 (coincident coarse coordinates) the host loop runs instead;
 * *used_device (may be NULL) tells which ran.  embed uses this form. */
int ge_radius_step_device(ge_ctx* ctx, int m, double* coords_A, double* r_A, int dim,
                          int coarse_is_base, int mc, const int* ptc_indptr,
                          const int* ptc_indices, const double* coords_Ac, const double* r_Ac,
                          const int* ac_indptr, const int* ac_indices, int* used_device);
/* The device rounds of the last ge_radius_step_device on ctx: how many ran and the
 * largest number of events popped in one of them (both 0 when no round ran: no
 * events, or the host loop ran instead). */
int ge_radius_info(const ge_ctx* ctx, int* rounds, int* max_pops);

/* ---- multi-GPU: one process per GPU, a communicator per context ----
 * The reference has no multi-GPU path (it is OpenMP on one node); these entry
 * points shard the same computations across ranks and return
 * the same bits on every rank as the single-GPU calls:
 *   - forceAtlas: contiguous row shards + one all-gather of the fp64
 *     coordinates per iteration (include/forceatlas.hpp:146-270 reads all
 *     coordinates of the previous iteration, nothing else is global: :228, :242);
 *     levels small enough for the fused single-launch kernels run as replicas.
 *   - forceAtlasMultilevel: aggregates dealt to ranks by cost (longest
 *     processing time first), no exchange during the iterations (:454, :462 read
 *     only the frozen coarse coordinates), one all-gather of the members'
 *     coordinates at the end.
 *   - P^T A P: coarse rows dealt to ranks in contiguous blocks of equal expanded
 *     work, one all-gather of the coarse rows.
 * A communicator is RCCL (ncclCommInitRank over xGMI: ge_comm_unique_id on
 * rank 0, shipped to the others out of band) or a caller transport (host
 * all-gather callback, e.g. MPI or gloo; data are staged through host memory).
 * Every rank passes the same inputs; collective calls must be made by all ranks
 * in the same order. */
#define GE_COMM_ID_BYTES 128
typedef struct ge_transport {
  void* user;
  /* All-gather of equal blocks: recv (nranks * bytes, rank-major) receives every
   * rank's `bytes` bytes of send.  Host pointers.  Returns 0 on success. */
  int (*allgather)(void* user, const void* send, void* recv, unsigned long long bytes);
} ge_transport;

int ge_comm_unique_id(unsigned char* id /* GE_COMM_ID_BYTES */);
/* RCCL communicator on the context's device; collectives run on its stream. */
int ge_comm_create(ge_ctx* ctx, int nranks, int rank, const unsigned char* id, ge_comm** out);
int ge_comm_create_transport(ge_ctx* ctx, int nranks, int rank, const ge_transport* t,
                             ge_comm** out);
int ge_comm_info(const ge_comm* comm, int* nranks, int* rank, int* is_rccl);
int ge_comm_destroy(ge_comm* comm);

/* Row shard of rank `rank`: rows [*row_begin, *row_end) of n, blocks of
 * *rows_per_rank = ceil(n / nranks) rows (coordinate buffers hold
 * nranks * rows_per_rank rows so every rank's block has the same size). */
int ge_row_shard(int n, int nranks, int rank, int* row_begin, int* row_end, int* rows_per_rank);
/* In-place all-gather of rank blocks of a device coordinate array
 * d_x[nranks * rows_per_rank * dim]: rank r contributes rows
 * [r * rows_per_rank, (r + 1) * rows_per_rank). */
int ge_allgather_coords(ge_comm* comm, double* d_x, long long rows_per_rank, int dim);
/* Deal aggregates to ranks by cost s(s-1) + (CSR entries of the members, when
 * indptr != NULL): descending cost (ties: lower id) to the least-loaded rank
 * (ties: lower rank).  owner[m] receives each aggregate's rank.  Host only. */
int ge_assign_aggregates(int m, const int* pt_indptr, const int* pt_indices, const int* indptr,
                         int nranks, int* owner);
/* After every rank wrote the coordinates of the members of its own aggregates
 * into d_x (n * dim, fine-vertex order; e.g. ge_faml_plan_run of a subset plan),
 * every rank holds all of them.  h_owner: ge_assign_aggregates' result;
 * h_pt_indptr / h_pt_indices: P_T on the host. */
/* ge_assign_aggregates with the giant aggregates split (owner -1): those with at
 * least min_members members (min_members > 0), none (0), or (< 0) those whose
 * ordered pairs exceed half a rank's average load (GE_DIST_SPLIT_MIN overrides). */
int ge_assign_aggregates_split(int m, const int* pt_indptr, const int* pt_indices,
                               const int* indptr, int nranks, int min_members, int* owner);
int ge_allgather_members(ge_comm* comm, double* d_x, int dim, int m, const int* h_pt_indptr,
                         const int* h_pt_indices, const int* h_owner);

/* Sharded forms of ge_force_atlas, ge_force_atlas_ml, ge_ptap and ge_embed (same
 * arguments, the context is the communicator's).  Results are identical on
 * every rank and bit-identical to the single-GPU calls. */
int ge_force_atlas_dist(ge_comm* comm, int n, const int* indptr, const int* indices,
                        const double* data, int dim, double* coords, int init_random,
                        int iterations, const ge_fa_params* p);
/* ge_layout_energy over row shards as ge_force_atlas_dist's: one all-gather of the per-row
 * values, then every rank sums all n rows with the one-GPU call's kernel, so rows and
 * totals have that call's bits on every rank. */
int ge_layout_energy_dist(ge_comm* comm, int n, const int* indptr, const int* indices,
                          const double* data, int dim, const double* coords,
                          const ge_fa_params* p, double* rows, double* totals);
int ge_force_atlas_ml_dist(ge_comm* comm, int n, const int* indptr, const int* indices,
                           const double* data, int m, const int* pt_indptr,
                           const int* pt_indices, const int* vertex_A, const double* coords_A,
                           const double* r_A, double* coords, int dim, int iterations,
                           const ge_fa_params* p);
int ge_ptap_dist(ge_comm* comm, int n, const int* indptr, const int* indices, const double* data,
                 int m, const int* pt_indptr, const int* pt_indices, ge_csr** out);
int ge_embed_dist(ge_comm* comm, int levels, const int* a_n, const int* a_off,
                  const int* a_nz_off, const int* a_indptr, const int* a_indices,
                  const double* a_data, const int* p_rows, const int* p_off,
                  const int* p_nz_off, const int* p_indptr, const int* p_indices, int dim,
                  int base_iterations, int ml_iterations, int print_progress,
                  const ge_fa_params* p, double* coords_out);

/* ---- alternative embedder ----
 * Replaces partition::embedViaMinimization(A, d, coords, ITER) (include/embed.hpp:22-23,
 * src/embed.cpp:341-559): `iterations` Gauss-Seidel sweeps of a per-vertex line
 * search towards the 2d unit directions, then centring and scaling.  coords:
 * n*dim in/out; init_random != 0 first draws U(-1,1) from mt19937(seed) (the
 * reference's empty-coords branch, :353-361).  Edge weights are not read (the
 * reference ignores them).  Host code (a single call is a chain of serial n-term
 * sums); the 2d directions run on OpenMP threads.
 * anyToMultilevel / embedVia / embedViaMultilevel (src/embed.cpp:23-338) are
 * header-only in graph-embed_amd/include/embed.hpp on top of this ABI. */
int ge_embed_via_minimization(int n, const int* indptr, const int* indices, int dim,
                              double* coords, int init_random, unsigned seed, int iterations);

/* Replaces anyToMultilevel(embedViaMinimization)(A, P_T, v_A, coords_A, r_A, coords, d)
 * (src/embed.cpp:23-83 over :341-559): per aggregate of P_T, `iterations` sweeps of
 * the minimiser from a zero start on the members' internal edges, the result
 * normalised by its largest norm and placed at coords_A[a] + r_A[a] * (x / max).
 * iterations: the reference's two-argument overload uses 1000.  With a context the
 * whole level is one batched device call (graph-embed_amd/csrc/ge_minimize_dev.hip)
 * when the rows of A and of P_T are strictly ascending and dim <= 4; ctx == NULL,
 * GE_MINIMIZE_HOST=1 or other inputs: the host path.  Same bits either way.  P_T
 * must list every fine vertex once and vertex_A must be its inverse.  An aggregate
 * with one member or without internal edges ends at NaN, as in the reference.
 * classes (may be NULL) receives the aggregates that ran packed (one lane per
 * direction), one wave per direction, and on the host (all of them on the host
 * path; on the device path those beyond the LDS capacity), then the path (0 host,
 * 1 device).  GE_MIN_PACK_MAX (largest packed aggregate, 0..64), GE_MIN_LDS_BYTES
 * (LDS capacity, at most the device's) and GE_MIN_WAVES (waves of a block) override
 * the class rule.  Diagnostics; the results do not depend on them. */
int ge_embed_via_minimization_ml(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                                 int m, const int* pt_indptr, const int* pt_indices,
                                 const int* vertex_A, const double* coords_A, const double* r_A,
                                 int dim, int iterations, double* coords, int* classes);

/* The reference's initial-coordinate stream: the first `count` values of
 * uniform_real_distribution<double>(-1,1) over mt19937(seed) (libstdc++). */
int ge_uniform_stream(unsigned seed, long long count, double* out);

/* Diagnostics: checks on the device that the strict kernels' shared-reciprocal
 * division (graph-embed_amd/csrc/ge_math.hpp) returns the same bits as IEEE
 * division for `samples` random and adversarial operand triples. */
int ge_selftest_math(ge_ctx* ctx, long long samples, unsigned long long seed,
                     long long* mismatches);

/* Diagnostics: the production helpers of the strict kernels on the caller's own
 * operands, one device thread per case, raw result bits back -- so that a test can
 * compare them with a correctly rounded reference and name a failing operand.  `in`
 * holds `count` rows of doubles, `out` receives `count` rows of bit patterns:
 *   GE_MATH_SQRT  in  s                     out sqrt_normal(s), the compiler's sqrt(s)
 *   GE_MATH_DIV   in  n, d                  out div_by(n, d, recip_of(d)), n / d
 *   GE_MATH_PAIR  in  s, n, c               out pair_den(s): dis, div_by_nz(n, rdis),
 *                                               div_by_nz(c, rdd), n / dis, c / (dis * dis)
 *   GE_MATH_REP   in  x_i[dim], x_j[dim],   out rep_term<dim, true, false>[dim],
 *                     deg_i + 1, deg_j + 1,     rep_term<dim, false, false>[dim]
 *                     repel                     (dim = 1..4; ignored by the other ops)
 * (graph-embed_amd/csrc/ge_math.hpp, ge_pair.hpp).  The operands are used as given:
 * the domain checks of the kernels (coord_ok, weight_ok) are the caller's. */
enum { GE_MATH_SQRT = 0, GE_MATH_DIV = 1, GE_MATH_PAIR = 2, GE_MATH_REP = 3 };
int ge_math_cases(ge_ctx* ctx, int op, int dim, long long count, const double* in,
                  unsigned long long* out);

/* ---- synthetic inputs (bench / tests) ----
 * Graph500 R-MAT (0.57, 0.19, 0.19, 0.05) with a counter-based SplitMix64
 * generator (definition: tests/graphs.py), symmetrised, deduplicated, unit
 * weights; and the largest connected component as examples/embedder.cpp:35-93. */
int ge_rmat_csr(int n, long long draws, unsigned long long seed, ge_csr** out);
int ge_largest_component(int n, const int* indptr, const int* indices, const double* data,
                         ge_csr** out);
/* The same two on the device (graph-embed_amd/csrc/ge_graph.hip), same results:
 * R-MAT by counter-based generation + radix sort + compaction, lcc != 0 returns
 * its largest connected component (hooking + pointer jumping, vertices renumbered
 * in ascending original id, examples/embedder.cpp:35-93). */
int ge_rmat_csr_device(ge_ctx* ctx, int n, long long draws, unsigned long long seed, int lcc,
                       ge_csr** out);
int ge_largest_component_device(ge_ctx* ctx, int n, const int* indptr, const int* indices,
                                const double* data, ge_csr** out);
/* The last of these two calls on ctx: the items per library sort or scan call
 * (GE_GRAPH_CHUNK, default 2^28), the row-range segments the R-MAT keys were sorted
 * in (0: one sort of all keys), the scans it ran and the library calls they took
 * (scan_calls > scans: a scan ran in chunks). */
int ge_graph_info(const ge_ctx* ctx, long long* chunk, int* sort_segments, int* scans,
                  int* scan_calls);

#ifdef __cplusplus
}
#endif
#endif /* GE_H */
