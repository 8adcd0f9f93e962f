/*
 * vet.h — C-ABI of the MI355X-native viewport -> Fibonacci-tile -> entropy engine.
 *
 * The reference (IamArmanNikkhah/viewport-entropy-toolkit) is pure Python and has
 * no FFI layer; its boundary for this path is the Python API.  This library sits
 * underneath a drop-in of that API and is bound with ctypes.
 * Each entry point names the reference code it replaces; paths are relative to
 * /root/reference/src/viewport_entropy_toolkit/.
 *
 * Conventions
 *   - plain C symbols, plain pointers and sizes; no C++ or torch types;
 *   - every function returns 0 on success or a negative VET_ERR_* code;
 *     vet_last_error() gives the thread-local message of the last failure;
 *   - the caller owns every buffer; the library keeps no caller pointer after a
 *     call returns (device inputs of an asynchronous call must stay alive until
 *     the stream has been synchronised);
 *   - sample arrays are FRAME-MAJOR: element (frame f, user u) is at [f*U + u],
 *     so one frame's users are contiguous (this is the dense form of the
 *     reference's ``vectors_df``: one row per frame, one column per user);
 *     an absent sample (reference: ``None`` cell) is NaN in mu or mv, or id -1;
 *   - "d_" parameters are device pointers, "h_" parameters are host pointers;
 *   - ``stream`` is a hipStream_t passed as void*.  NULL selects the CONTEXT'S OWN stream
 *     (hipStreamNonBlocking: not ordered against the null stream) — it is NOT the null stream.
 *     To run on the legacy default stream (what torch calls its default stream, handle 0) pass
 *     VET_STREAM_LEGACY; any other value is used as the hipStream_t it is.
 *     Device-pointer entry points only enqueue work; they do not synchronise.  A context — and
 *     every plan of it — is single-threaded and must not be in use on two streams at once: its
 *     scratch (the K > 1 workspace, the transition scratch, the resolve list of an FP table) is
 *     shared by all calls, so calls on different streams must be synchronised in between.
 *     (Batch descriptors are not part of that scratch: each batch call stages them in its own
 *     slot of an event-guarded ring, so back-to-back batch calls need no synchronisation.)  A plan's tables are complete (stream synchronised) when the
 *     call that built them returns; a result handle (vet_result) may outlive its context.
 *   - there is no CPU fallback: without a gfx950 device vet_create() fails.
 */
#ifndef VET_H_
#define VET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VET_VERSION 141 /* 0.1.4: tile_weights values at the reference's precision under every formulation
                           (+ vet_plan_set_raw_weights); batch descriptors in an event-guarded ring;
                           0.1.4.1: vet_device_pci_bus_id; vet_plan_set_fp64 (formulation 4, `dtable`) added
                           without a new number: existing callers see no change; the vet_heatmap_* entry points
                           (per-frame tile-attention heatmaps), the vet_tiling_* entry points
                           (tilings drawn on the unit sphere) and vet_heatmap_render_counts /
                           vet_heatmap_render_transition_result (heatmaps of transition results) and
                           vet_heatmap_create_latlon / vet_heatmap_render_binned(_host) (lat/lon cell
                           heatmaps of naive plans) added the same way; so were vet_window_rows and the
                           vet_spatial_entropy_windowed* entry points (pooled entropy of sliding frame windows), and
                          then the vet_transition_entropy_windowed* entry points (pooled transitions of windows of pairs) and
                          the vet_user_entropy* entry points (each viewer's own histogram over time), and then the
                          vet_user_divergence* entry points (a U x U Jensen-Shannon matrix between viewers per window), and
                          then the vet_window_divergence* entry points (a lag band of Jensen-Shannon distances between windows) and the
                          vet_crowd_divergence* entry points (each viewer's Kullback-Leibler divergence from the pooled crowd), and
                          then the vet_bootstrap_entropy* entry points (confidence bands from viewers resampled with replacement)
                          and vet_bootstrap_counts_host, and then the vet_group_divergence* entry points (a permutation test
                          of the attention divergence between two audiences) and vet_group_labels_host, and then the
                          vet_coverage* entry points (top-k tile sets per window and the share of later windows they hold), and
                          then the vet_transition_markov* entry points (tile-to-tile transition counts per window: entropy rate,
                          stationary and destination entropy, mutual information at a lag, stay share), and then the
                          vet_head_motion* entry points (angular speed of the heads: moments, exact quantiles and a histogram of the
                          angle between a viewer's directions `lag` frames apart, per window and per viewer), and then the
                          vet_dispersion* entry points (audience dispersion: the angle between two viewers' directions in one
                          frame over all pairs, per window and per viewer), and then the vet_saliency* entry points (saliency
                          maps: the spherical kernel density of a window's viewing directions on an equirectangular map, with its
                          mass, peak, entropy and effective area, per window and per viewer) and vet_test_saliency_tile, and then
                          the vet_saliency_similarity* entry points (CC, SIM, JSD, KL and NSS between the maps of two audiences), and
                          then the vet_congruency* entry points (each viewer's leave-one-out saliency score per window); the
                          vet_saliency_score* entry points (AUC, NSS, information gain, CC, SIM, JSD and KL of a predicted map)
                          were added under the same number, and so were the vet_viewer_clusters* entry points (the connected
                          components of the viewers linked by the angle between their directions, per window) and
                          vet_test_cluster_tile, and the vet_fixations* entry points (fixation and tile-dwell events: per
                          viewer the maximal runs of frames with a steady viewport, per window and per viewer) and
                          vet_test_fixation_chunk */
#define VET_STREAM_LEGACY ((void *)1) /* == hipStreamLegacy: the null stream with legacy ordering */
/* Policy 0 of vet_plan_set_table_policy: a weighted call gathers from the direction weight table iff it holds at least this
 * many samples per direction of the plan's direction table.  Measured (profiles/r06/first_call.txt, grid_sensitivity.txt):
 * building a direction's row costs what the sweep spends on ~20 samples; with the alias table built on the device the table's
 * FIRST call costs at most 1 ms more than the sweep's on 100x200 / 200x400 grids and 27 % more on 3840x1920, and every later
 * call of the plan is 3.7-10x cheaper than the sweep — at 2 samples per direction the table has paid for itself by the
 * plan's second (large grids) to tenth (config-2-sized videos) call.  Rounds 1-5 used 8: the alias table was a host hash map
 * then, which made a first call 1.5 s on a 3840x1920 grid. */
#define VET_TABLE_SAMPLES_PER_DIRECTION 2

enum {
    VET_OK = 0,
    VET_ERR_INVALID = -1,   /* bad argument (maps to ValueError / ValidationError) */
    VET_ERR_DEVICE = -2,    /* HIP failure / no device (maps to RuntimeError) */
    VET_ERR_RANGE = -3,     /* a 2dmu/2dmv value outside [0,1]  (reference: ValidationError,
                               utilities/data_utils.py:256-257) */
    VET_ERR_EMPTY = -4,     /* a frame without any (common) user (reference: ValidationError
                               entropy_utils.py:170 / ZeroDivisionError entropy_utils.py:299) */
    VET_ERR_UNSUPPORTED = -5
};

typedef struct vet_ctx vet_ctx;   /* one device + stream + scratch; one per thread */
typedef struct vet_plan vet_plan; /* device tables for one analyzer configuration */

/* ---- library / device ---------------------------------------------------- */
int vet_version(void);
const char *vet_last_error(void);
int vet_device_count(void);
int vet_create(int device_id, vet_ctx **out);
int vet_destroy(vet_ctx *ctx);
int vet_synchronize(vet_ctx *ctx);
/* The device a context computes on, as its PCI bus id ("0000:05:00.0"; buf of len >= 16): what a rank of a
 * multi-GPU job (one process per video, README.md:108-120) reports so that a job can show that its N ranks
 * sit on N distinct devices (bench.py's per_rank block; _dist refuses two ranks of an RCCL job on one device). */
int vet_device_pci_bus_id(vet_ctx *ctx, char *buf, int len);
/* Per-kernel timing with hipEvents on the launch stream (bench.py's roofline leg). */
int vet_profile_enable(vet_ctx *ctx, int on);
/* Test switch, not a tuning knob: on != 0 makes the tables that plans of this context build from now on keep every row whole
 * (cap = stride, no overflow table; vet_plan_table_cap) — the layout of plans where no cap qualifies, so that a test can
 * compare the two layouts in one process.  Results are bit-identical either way. */
int vet_test_no_row_cap(vet_ctx *ctx, int on);
/* Test switch, not a tuning knob: on != 0 makes the table launches of this context's plans read the 8-byte direction record
 * (row, nearest tile, row meta) where a capped plan also has the 4-byte one (vet_plan_record_bytes).  Read at every launch,
 * so one plan runs both kernels in one process.  Results are bit-identical either way. */
int vet_test_rec8(vet_ctx *ctx, int on);
/* Test switch, not a tuning knob: on != 0 makes vet_user_transition_entropy* run rows of up to 64 frame pairs through the hash
 * kernel of the longer rows (k_user_transition) instead of k_user_transition_wave.  Read at every launch, so one plan runs
 * both kernels in one process.  The two sum a row's cells in different orders: results agree to rounding, not bit for bit. */
int vet_test_user_transition_hash(vet_ctx *ctx, int on);
/* Test switch, not a tuning knob: rows > 0 makes vet_user_divergence* build the viewers' histograms `rows` rows at a time
 * instead of as many as its workspace budget holds, so that a small input runs several chunks; 0 restores the default.  Read at
 * every launch.  Results are bit-identical whatever the value. */
int vet_test_divergence_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes vet_window_divergence* take `rows` pair rows per histogram chunk (plus the halo
 * of max_lag rows) instead of as many as its workspace budget holds, so that a small input runs several chunks and the halo
 * crosses them; 0 restores the default.  Read at every launch.  Results are bit-identical whatever the value. */
int vet_test_window_divergence_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes vet_crowd_divergence* take `rows` rows per chunk instead of as many as its
 * workspace budget holds, so that a small input runs several chunks; 0 restores the default.  Read at every launch.  Results are
 * bit-identical whatever the value. */
int vet_test_crowd_divergence_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes vet_bootstrap_entropy* build the viewers' histograms `rows` rows at a time instead
 * of as many as its workspace budget holds, so that a small input runs several chunks; 0 restores the default.  Read at every
 * launch.  Results are bit-identical whatever the value. */
int vet_test_bootstrap_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes vet_group_divergence* build the viewers' histograms `rows` rows at a time instead
 * of as many as its workspace budget holds, so that a small input runs several chunks; 0 restores the default.  Read at every
 * launch.  Results are bit-identical whatever the value. */
int vet_test_group_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes vet_coverage* take `rows` rows per histogram chunk (plus the halo of max_lag
 * rows) instead of as many as its workspace budget holds, so that a small input runs several chunks and the halo crosses them; 0
 * restores the default.  Read at every launch.  Results are bit-identical whatever the value. */
int vet_test_coverage_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: rows > 0 makes the chunked shape of vet_transition_markov* (window * n_users > 32768) build the
 * dense matrices of `rows` rows per pass instead of as many as its workspace budget holds, so that a small input runs several passes;
 * 0 restores the default.  Read at every launch.  Results are bit-identical whatever the value. */
int vet_test_markov_chunk_rows(vet_ctx *ctx, int rows);
/* Test switch, not a tuning knob: n > 0 lowers the most values of a row that one workgroup of vet_head_motion* takes from 16384 to
 * n (rounded down to a multiple of 1024, at least 1024, at most 16384), so that small inputs reach the chunked shape; 0 restores the
 * default.  Read at every launch.  Results are bit-identical whatever the value. */
int vet_test_motion_lds_values(vet_ctx *ctx, int n);
/* Test switch, not a tuning knob: n > 0 lowers the most viewers of a frame that k_dispersion_pairs (vet_dispersion*) stages in LDS at
 * a time from 1024 to n (at most 1024), so that a small audience runs several tiles; 0 restores the default.  Read at every launch.
 * Results are bit-identical whatever the value. */
int vet_test_dispersion_tile(vet_ctx *ctx, int n);
/* Test switch, not a tuning knob: n > 0 lowers the most list entries of a row that k_saliency_map (vet_saliency*,
 * vet_saliency_similarity*), k_saliency_points (vet_saliency_similarity*: the other audience's list) and k_congruency_points
 * (vet_congruency*: the pooled list) stage in LDS at a time (default and upper limit 1024; 0 restores the default).  Read at every launch; results do not depend on it. */
int vet_test_saliency_tile(vet_ctx *ctx, int n);
/* Test switch, not a tuning knob: rows > 0 makes vet_viewer_clusters* take at most `rows` rows per pass instead of as many as its
 * 256 MB budget of link words holds, and tile > 0 lowers the most partners of one workgroup of k_cluster_links from 128 to `tile`,
 * so that a small input runs several passes and several partner tiles; 0 restores a default.  Read at every launch, nowhere from
 * the environment.  Results are bit-identical whatever the values. */
int vet_test_cluster_tile(vet_ctx *ctx, int rows, int tile);
/* Test switch, not a tuning knob: n > 0 lowers the frames of one chunk of the walk of vet_fixations* over a viewer's frames from 1024
 * to n (a multiple of 4, the frames of one thread; at most 1024), so that the seams between chunks, and between the waves of a
 * chunk, show on videos of a few dozen frames; 0 restores the default.  Read at every launch, nowhere from the environment.
 * Results are bit-identical whatever the value. */
int vet_test_fixation_chunk(vet_ctx *ctx, int n);
int vet_profile_reset(vet_ctx *ctx);
/* kernel ids: 0 k_grid_dirs, 1 k_nearest_lut, 2 k_spatial (any variant), 3 k_transition,
 *             4 k_finalize, 5 k_wtab (direction weight table build),
 *             6 k_weights (the weights pass: k_weights_gather over the plan's exact FP64 weight rows, or the precise sweep in
 *               weights-only mode where those do not fit: the d_weights output / fetched weight rows) */
int vet_profile_get(vet_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
const char *vet_kernel_name(int kernel_id);

/* ---- device memory helpers (for hosts without torch) --------------------- */
int vet_malloc(vet_ctx *ctx, size_t bytes, void **d_ptr);
int vet_free(vet_ctx *ctx, void *d_ptr);
int vet_memcpy_h2d(vet_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int vet_memcpy_d2h(vet_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* ---- plan: what SpatialEntropyAnalyzer.__init__ + AnalyzerConfig hold ----- */
typedef struct vet_plan_desc {
    /* Quantiser of process_viewport_data + format_trajectory_data + Vector.from_spherical
     * (utilities/data_utils.py:243-286, 390-397; data_types.py:204-216) as per-axis tables
     * built by the host with the reference's own float operations:
     *   lon axis, px = 0..W : cos(theta), sin(theta), theta = radians(lon(px))
     *   lat axis, py = 0..H : sin(phi),   cos(phi),   phi   = radians(90 - lat(py))
     * The device forms x = round6(sin(phi)*cos(theta)), y = round6(sin(phi)*sin(theta)),
     * z = round6(cos(phi)).  Leave all four NULL and set dir_table for an explicit table. */
    int video_width, video_height;
    const double *h_lon_cos, *h_lon_sin; /* [W+1] */
    const double *h_lat_sin, *h_lat_cos; /* [H+1] */
    /* Alternative to the axis tables: explicit direction table (rounded Vector xyz), used by
     * the operator-level compute_spatial_entropy / compute_transition_entropy shims
     * (utilities/entropy_utils.py:147-151, 213-219) where callers pass arbitrary Vectors. */
    const double *h_dir_table; /* [n_dirs*3] or NULL */
    int64_t n_dirs;
    /* Lattices: generate_fibonacci_lattice(tile_count) per AnalyzerConfig.tile_counts entry
     * (analyzers/spatial_entropy.py:63-66), as rounded Vector xyz. */
    int n_lattices;                 /* K >= 1 */
    const int *n_tiles;             /* [K]  n_k = 2*floor(tile_count/2)+1 */
    const double *const *h_tiles;   /* K pointers to [n_k*3] */
    const double *h_max_entropy;    /* [K]  -n*(1/n)*log2(1/n), entropy_utils.py:201-203 */
    /* EntropyConfig (utilities/entropy_utils.py:20-38) */
    double fov_angle;               /* degrees, (0,360] */
    double max_angular_distance;    /* np.radians(fov_angle/2), entropy_utils.py:124 */
    double power_factor;            /* > 0 */
    int use_weight_distribution;
    /* Optional "binned" lattices (NULL = none): h_bin_lut[k] != NULL replaces lattice k's
     * nearest-tile search by a caller-supplied direction -> bin table [n_dirs] with n_tiles[k]
     * bins (h_tiles[k] is then ignored).  This is the naive lat/lon tiling of
     * compute_naive_spatial_entropy (utilities/entropy_utils.py:383-452): every user adds 1 to
     * its bin; use_weight_distribution only selects the normaliser (log2 of h_max_entropy's n
     * always, vs. log2(users) when users <= n). */
    const uint16_t *const *h_bin_lut;
    /* [K] or NULL: the tile count the normaliser compares the user count with when it differs from
     * the number of histogram bins (naive tiling: (180/h)*(360/w) tiles, but lon = 180 / lat = 90
     * open one more bin column / row). */
    const int *n_norm_tiles;
} vet_plan_desc;

int vet_plan_create(vet_ctx *ctx, const vet_plan_desc *desc, vet_plan **out);
int vet_plan_destroy(vet_plan *plan);
int64_t vet_plan_n_dirs(const vet_plan *plan);
/* Weighted spatial mode (calculate_tile_weights, entropy_utils.py:108-144) has five formulations:
 *   0 table    direction weight table, built once per plan and gathered per distinct direction of a
 *              frame (memory bound); 32-bit block-floating-point weights, 64-bit integer histograms
 *   1 sweep    every sample sweeps every tile (FP64 VALU bound); 2^-52 fixed-point integer histograms
 *   2 precise  the sweep with the exact weights in FP64 histograms, in the reference's summation order
 *   3 ftable   the table with FP32 weights (2^-24 relative each, scaled by their row's exponent) in FP64
 *              histograms: |dH|/H <= 1.2e-7 for every frame whatever the weights' dynamic range
 *   4 dtable   FP64 from start to end (plans with vet_plan_set_fp64 only): per frame, the users' exact FP64 weight rows
 *              of every lattice (the rows the tile_weights pass gathers, built once per plan and lattice) summed in FP64
 *              histograms in a fixed order — the users in column order within each of NW contiguous shares, the shares
 *              in order, NW as for tile_weights —, then the reference's -sum q log2 q over the keys: bit-identical run
 *              to run, under any frame split and between the ids and the grid entry points; lattice 0's sums ARE the
 *              tile_weights values (the call that asks for both runs one pass).  Its NaN frames are the reference's
 *              with no special case (a key whose sum is 0.0 gives 0 * log2 0)
 * The integer formulations (0, 1) are order independent (bit-identical run to run, under any user
 * permutation, frame split or GPU count).  They are only used where a bound computed from the plan's
 * own rows proves their deviation from exact arithmetic <= 1e-7 relative for EVERY possible frame
 * (k_row_stats; the contract is 1e-6); plans outside that — FoV cones narrower than the lattice
 * spacing, large power factors — run `ftable` (calls large enough for a table) or `precise`; those two
 * sum in FP64 in a fixed order: `ftable` sorts every frame's list of distinct rows, gives every wave a histogram
 * of its own and adds those in wave order (bit-identical run to run, under any user permutation of frames of
 * <= 2048 users, frame split or GPU count — as measured on gfx950: where two rows of one wave instruction hit the
 * same tile the result also rests on the LDS servicing the lanes of a ds_add_f64 in lane order, which the hardware
 * does and the ISA does not promise; tests/test_hip_contract.py and tools/repeat_check.py are the guard);
 * `precise` sums the users in column order, as the reference does
 * (as the resolver of `ftable`: in ascending direction order).
 * The reference's NaN frames: every tile with distance < fov/2 is a key of the reference's per-frame dict,
 * also when ((max - d) / max) ** power_factor underflows to exactly 0.0 (entropy_utils.py:131-135), and a key
 * whose summed weight is 0.0 (or underflows against the frame total) makes the entropy NaN = 0 * log2 0
 * (:195-198).  Plans with such weights (below 2^-1048; power_factor >~ 80 on the default grids) never use an
 * integer formulation; `precise` keeps the exact key set, and `ftable` keeps every in-FoV tile without an FP32
 * value as a marker entry and hands the frames those markers decide to `precise` inside the same call.
 * Which formulation a call uses is a pure function of the plan and the call's shape, never of the
 * plan's history: policy 0 = table iff the call (or batch) holds >= VET_TABLE_SAMPLES_PER_DIRECTION samples per direction of the
 * plan's direction table, +1 = table whenever it is inside the contract and fits, -1 = never table.
 * vet_plan_table_stride: row length of lattice k's table (of the plan's fused table — one row per direction over
 * all lattices — where that is the one in use), 0 = not built (yet), -1 = does not fit.
 * vet_plan_set_fp64: on != 0 restricts the plan's weighted Fibonacci lattices to FP64 arithmetic end to end: where the
 * policy's rule asks for a table and lattice k's exact rows exist (they do not when the plan's rows would exceed 8 GB or a
 * quarter of the free device memory, or under VET_NO_EXACT_ROWS), `dtable`; `precise` otherwise — never `table`, `sweep` or
 * `ftable`.  Binned lattices and unweighted plans count integers and are unaffected.  The batch entry points run an fp64
 * plan video by video through vet_spatial_entropy (no batched launch).  on = 0 restores the default choice.
 * vet_plan_last_formulation: formulation lattice k used in the plan's last weighted call (-1 none).
 * vet_plan_error_bounds: the proven relative entropy error bounds of lattice k for the table and the
 * sweep (at <= 1024 users) formulations; inf = a frame exists whose entropy no fixed point resolves. */
int vet_plan_set_table_policy(vet_plan *plan, int policy);
int vet_plan_set_fp64(vet_plan *plan, int on);
/* tile_weights VALUES (the d_weights / h_weights outputs and the weight rows of a vet_result; calculate_tile_weights and
 * the accumulation of compute_spatial_entropy, utilities/entropy_utils.py:131-136, 190-192).  Whatever formulation
 * produces the entropy, they are the reference's: exact FP64 weights (ocml acos / pow), summed over the users in column
 * order within each of NW contiguous shares of the users (NW = 4, 2 or 1 by lattice size and LDS), the shares added in order —
 * deterministic, within 1e-9 relative of the reference's single sequential sum, not bit-equal to it —, by a weights pass of its own: a gather of
 * exact FP64 weight rows built once per plan on the first request (the `precise` sweep in weights-only mode where those
 * rows do not fit the device).  Only calls that ask for the weights pay for it (config-3 shape: 2.8 ms for all 30 000
 * frames; a vet_result computes the rows of a fetched block, 256 frames 0.2 ms), and the entropy path is untouched.  on != 0 returns the formulation's own histogram instead (block-floating-point / FP32 / 2^-52 fixed-point
 * weight sums: at most n_users * 2^-33 of the row's scale off under the table): a diagnostic for the table layouts. */
int vet_plan_set_raw_weights(vet_plan *plan, int on);
int vet_plan_table_stride(const vet_plan *plan, int lattice);
/* rows of a weight table = distinct directions up to the lattice's mirror symmetry (0 before the first table exists):
 * a table takes (rows + 1) * stride * 6 bytes */
int64_t vet_plan_table_rows(const vet_plan *plan);
/* Row cap of lattice k's own table (0 = no such table): integer tables of one-lattice plans keep `cap` entries per row — the
 * smallest multiple of 64 that at most 1/32 of the rows exceed — and the tails of the longer rows in one 64-slot block each
 * of an overflow table, numbered in row order (*overflow_rows of them, nullable; an all-zero row follows the last).
 * cap == stride; a table whose rows are all whole has no overflow table (also forced by vet_test_no_row_cap). */
int vet_plan_table_cap(const vet_plan *plan, int lattice, int64_t *overflow_rows);
/* Bytes of the per-direction record that the plan's table launches with the set of distinct rows (frames of >= 128 users)
 * gather per sample: 4 = the compact record (row 15 bits | mirrored | nearest tile 10 bits | -shift 5 bits | row continues in
 * the overflow table), built beside the 8-byte one for capped one-lattice tables of fewer than 2^15 rows and at most 2^10
 * tiles; 8 otherwise (also under vet_test_rec8); 0 = lattice 0 has no table with records yet.  vet_plan_read_records copies
 * the compact records [n_dirs] to the host (an error where the plan has none). */
int vet_plan_record_bytes(const vet_plan *plan);
int vet_plan_read_records(vet_plan *plan, uint32_t *h_rec32);
int vet_plan_last_formulation(const vet_plan *plan, int lattice);
/* The table kernel (k_spatial_lut instantiation) and launch geometry of the plan's last table launch, as the launch decided
 * them: read-only introspection for tests, 0 before any table launch (formulations `table` and `ftable`; the other
 * formulations leave the word as it is).  Fields: */
#define VET_TK_LAUNCHED  0x00000001u /* a table kernel has been launched */
#define VET_TK_NB_SHIFT  1           /* bits 1..2: blocks of a capped row (1..3: the fixed-trip kernels), 0 = whole rows */
#define VET_TK_NB_MASK   0x3u
#define VET_TK_REC32     0x00000008u /* the 4-byte direction record (vet_plan_record_bytes) */
#define VET_TK_BUCKETED  0x00000010u /* bucket-ordered row lists */
#define VET_TK_DEDUP     0x00000020u /* the per-frame set of distinct rows */
#define VET_TK_IL        0x00000040u /* class-dealt (interleaved) rows */
#define VET_TK_OCC8      0x00000080u /* the instantiation bounded to 8 workgroups per CU */
#define VET_TK_FP_TABLE  0x00000100u /* FP32 table (`ftable`) */
#define VET_TK_FUSED     0x00000200u /* the plan's fused table: one row over all lattices */
#define VET_TK_NARROW    0x00000400u /* fused only: the 8-lane kernel (32-entry blocks), else the 16-lane one */
#define VET_TK_FROM_IDS  0x00000800u /* samples given as direction ids (vet_spatial_entropy_ids) */
#define VET_TK_BATCH     0x00001000u /* one launch over the videos of a batch */
#define VET_TK_CHUNKED   0x00002000u /* the users of a frame ran in more than one chunk (0 for a batch: per video there) */
#define VET_TK_FPW_SHIFT 16          /* bits 16..23: frames per workgroup (0 for a batch: per video there) */
#define VET_TK_FPW_MASK  0xFFu
uint32_t vet_plan_last_table_kernel(const vet_plan *plan);
int vet_plan_error_bounds(vet_plan *plan, int lattice, double *table_bound, double *sweep_bound);
/* Parity hooks: read back the device-built tables (synchronous). */
int vet_plan_read_dirs(vet_plan *plan, double *h_xyz /* [n_dirs*3] rounded Vector xyz */);
int vet_plan_read_nearest(vet_plan *plan, int lattice, int32_t *h_nearest /* [n_dirs] */);
/* lattice k's own weight table (every output nullable): mantissas and tiles [(rows+1)*stride], meta words [rows+1]
 * (entries of the main row in bits 0..11, bit 15 = the row continues in the overflow table, row shift from bit 16);
 * capped tables only: the overflow table [(overflow_rows+1)*64] and every row's block in it [rows] (0xFFFFFFFF = none) */
int vet_plan_read_table(vet_plan *plan, int lattice, uint32_t *h_w, uint16_t *h_tile, uint32_t *h_meta, uint32_t *h_ovf_w,
                        uint16_t *h_ovf_tile, uint32_t *h_ovf_of_row);

/* ---- hot path: SpatialEntropyAnalyzer.compute_entropy ---------------------
 * (analyzers/spatial_entropy.py:107-164 -> entropy_utils.py:147-211, 108-144, 89-106, 41-87)
 *   d_entropy [T]      mean over the plan's lattices of the normalised spatial entropy
 *   d_assign  [T*U]    nearest tile of lattice 0 per sample, -1 absent      (nullable)
 *   d_weights [T*n_0]  per-frame tile weight sums of lattice 0              (nullable)
 *                      at the reference's precision under every formulation (vet_plan_set_raw_weights);
 *                      -0.0 = the tile is a key of the reference's dict with the value 0.0 (in some
 *                      user's FoV, weight underflowed), +0.0 = no key
 *   d_present [T]      users present per frame                              (nullable)
 *   d_status  [2]      {bad, #frames without a user}; the call ADDS to it, the caller
 *                      zeroes it                                            (nullable)
 *                      bad: non-zero if and only if some sample is outside [0,1] (ids: at
 *                      or beyond the direction table); not the number of such samples   */
int vet_spatial_entropy(vet_plan *plan, const double *d_mu, const double *d_mv,
                        int n_users, int n_frames,
                        double *d_entropy, int32_t *d_assign, double *d_weights,
                        int32_t *d_present, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_spatial_entropy_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames,
                            double *d_entropy, int32_t *d_assign, double *d_weights,
                            int32_t *d_present, int32_t *d_status, void *stream);

/* ---- sliding-window spatial entropy: the frames of a window pooled into one histogram -----------
 * For window = w >= 1, stride = s >= 1 and n_frames = T >= w there are R = (T - w) / s + 1 rows (integer division;
 * vet_window_rows, < 0 for illegal arguments); row r covers frames [r*s, r*s + w).  Row r is, for every lattice of the plan,
 * what compute_spatial_entropy (utilities/entropy_utils.py:147-211; naive plans: compute_naive_spatial_entropy, :383-452)
 * returns for ONE dict that holds every present (frame, user) sample of those frames, frame-major then user order, then the
 * mean over the lattices as compute_entropy takes it (analyzers/spatial_entropy.py:142-156).  So, with `samples` = the present
 * samples of the window (not users):
 *   weighted: the keys are the tiles with distance < fov/2 of some sample of the window, the normaliser is log2(n); a key
 *     whose weights are all 0.0 makes the row NaN (0 * log2 0);
 *   unweighted and binned (naive) lattices: every sample adds 1 to its tile / bin; the normaliser is log2(n) if
 *     use_weight_distribution or samples > n, else log2(samples); one sample in the window gives the reference's NaN (0 / 0);
 *   a window without any present sample: NaN in d_entropy, 0 in d_samples and d_status[1] += 1 — what vet_spatial_entropy
 *     does with a frame without a user; the _host entry then returns VET_ERR_EMPTY (outputs are still written).
 * window = 1, stride = 1 is the per-frame series.
 *   d_entropy [R]
 *   d_weights [R*n_0]  lattice 0's pooled histogram, encoded and toleranced as vet_spatial_entropy's d_weights  (nullable)
 *   d_samples [R]      present samples of the window                                                            (nullable)
 *   d_status  [2]      {bad, #rows without a sample}; as vet_spatial_entropy: the call ADDS, the caller zeroes   (nullable)
 * Two stages; every frame's histogram is built once, whatever the overlap of the windows:
 *   1 per frame: weighted Fibonacci lattices — the `dtable` arithmetic: the users' exact FP64 weight rows (k_weights_gather,
 *     built once per plan and lattice) summed per frame in `dtable`'s order (above), [T][n_k] f64 per lattice; there is no
 *     other formulation, no error bound to check and no NaN hand-over: where a lattice's exact rows do not fit the device
 *     (vet_plan_set_fp64's rule) the call fails with VET_ERR_UNSUPPORTED.  Unweighted and binned lattices — the tile / bin
 *     of every sample, [T][U] i32 per lattice (k_window_tiles).  The call's scratch (those arrays, T * 4 bytes of frame
 *     counts and K * R * 8 bytes of per-lattice rows) is the context's grow-only workspace: no allocation in steady state;
 *   2 per row and lattice (k_window_entropy): weighted — the window's w frame histograms ADDED IN ASCENDING FRAME ORDER from
 *     the window's first frame, for every row anew (never a running sum with subtractions), then `dtable`'s epilogue in one
 *     wave; integer counts — a wave owns a run of consecutive rows, keeps the window's counts in LDS, adds the frames that
 *     enter and subtracts those that leave (exact), then the per-frame kernel's epilogue in one wave.
 * A row is therefore a pure function of the plan and the samples of its w frames: the same bits whatever stride selected
 * it, wherever its frames lie in the call, from run to run, and between the ids and the grid entry points.  With window = 1
 * a weighted plan gives the bits of the same plan under vet_plan_set_fp64 where that call runs `dtable`, and an unweighted /
 * binned plan gives the bits of vet_spatial_entropy where that runs k_spatial_u_lds (grid samples, n_users <= 4096, the
 * nearest-tile table in LDS; the other per-frame kernel takes log2(v / N) directly: same value within an ulp or two).
 * Limits: an integer-count lattice keeps one u32 per bin in LDS, so binned lattices of more than lds / 4 bins (40 832 on
 * gfx950; naive 1 x 1 degree cells have 65 341) are refused with VET_ERR_UNSUPPORTED.
 * VET_ERR_INVALID: window < 1, stride < 1, window > n_frames (and what vet_spatial_entropy refuses).
 * The kernels have no profile id of their own: stage 1 is charged to k_weights (weighted) / k_spatial (k_window_tiles),
 * stage 2 to k_finalize.  Asynchronous on `stream` like vet_spatial_entropy. */
int64_t vet_window_rows(int n_frames, int window, int stride);
int vet_spatial_entropy_windowed(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames,
                                 int window, int stride, double *d_entropy, double *d_weights, int32_t *d_samples,
                                 int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_spatial_entropy_windowed_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                                     double *d_entropy, double *d_weights, int32_t *d_samples, int32_t *d_status,
                                     void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE / VET_ERR_EMPTY when the status words are non-zero (outputs are
 * still written).  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_spatial_entropy_windowed_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids,
                                      int n_users, int n_frames, int window, int stride, double *h_entropy,
                                      double *h_weights, int32_t *h_samples);

/* ---- per-viewer spatial entropy: each user's own tile histogram over time ------------------------
 * The transposed question of the windowed call: not "how spread out is the audience over these frames" but "how much of the
 * sphere does this viewer visit".  For window = w, stride = s and n_frames = T there are R = vet_window_rows(T, w, s) rows per
 * user; row (u, r) covers frames [r*s, r*s + w) of user u.  Its value is, for every lattice of the plan, what
 * compute_spatial_entropy (utilities/entropy_utils.py:147-211; naive plans: compute_naive_spatial_entropy, :383-452) returns
 * for ONE dict that holds user u's present samples of those frames in ascending frame order, then the mean over the lattices
 * as compute_entropy takes it.  So, with `samples` = the user's present samples of the row:
 *   weighted: the keys are the tiles with distance < fov/2 of some sample of the row, the normaliser is log2(n); a key whose
 *     weights are all 0.0 makes the row NaN (0 * log2 0);
 *   unweighted and binned (naive) lattices: every sample adds 1 to its tile / bin; the normaliser is log2(n) if
 *     use_weight_distribution or samples > n, else log2(samples); one sample in the row gives the reference's NaN (0 / 0);
 *   a row in which the user has no sample: NaN in d_entropy, 0 in d_samples and d_status[1] += 1.  Viewers join and leave, so
 *     such rows are data, not errors: the _host entry does NOT turn them into VET_ERR_EMPTY.
 * window = n_frames is the whole video (R = 1).  Outputs are user-major:
 *   d_entropy [U][R]
 *   d_weights [U][R][n_0]  lattice 0's histogram of the row, encoded and toleranced as vet_spatial_entropy's d_weights (-0.0 =
 *                          key with the value 0.0, +0.0 = no key)                                                  (nullable)
 *   d_samples [U][R]       the user's present samples of the row                                                   (nullable)
 *   d_status  [2]          {bad, #rows without a sample}; the call ADDS, the caller zeroes                           (nullable)
 * Two stages:
 *   1 k_user_dirs: every sample is quantised once and its direction id written transposed, [U][T] i32 (-1 absent), through a
 *     64 x 64 LDS tile (both the [T][U] read and the [U][T] write are coalesced).  d_status[0] is raised as k_window_tiles
 *     raises it.  That array and, for plans of several lattices, K * U * R * 8 bytes of per-lattice rows are the context's
 *     grow-only workspace: no allocation in steady state;
 *   2 per (user, row) and lattice, over a contiguous slice of the user's ids.  Weighted Fibonacci lattices (k_user_entropy_w):
 *     one workgroup per row; its NW waves take contiguous shares of the row's frames, each adds the exact FP64 weight rows
 *     (`dtable`'s, built once per plan and lattice) of its frames IN ASCENDING FRAME ORDER into its own histogram, the waves'
 *     histograms are added in wave order, then `dtable`'s epilogue in one wave.  Every row is summed from scratch (window
 *     row-adds per row whatever the overlap); NW is 1 up to 64 frames per row, 2 up to 128, else 4 (fewer where NW * n * 8
 *     bytes of histograms do not fit the LDS) — a function of the window and the plan alone.  There is no other formulation:
 *     where a lattice's exact rows do not fit the device the call fails with VET_ERR_UNSUPPORTED.  Unweighted and binned
 *     lattices (k_user_entropy_c): a wave owns a run of consecutive rows of one user, keeps the counts (u32 per tile) in LDS,
 *     adds the frames that enter and subtracts those that leave (exact), then the windowed call's integer epilogue.
 * A row is therefore a pure function of the plan and of its own samples: the same bits whatever stride selected it, wherever
 * its frames lie in the call, whichever other users the call holds, from run to run, and between the ids and the grid entry
 * points.
 * Limits: as the windowed call's (n * 4 bytes of LDS for a counting lattice, n * 8 for a weighted one); U * R < 2^31.
 * VET_ERR_INVALID: window < 1, stride < 1, window > n_frames (and what vet_spatial_entropy refuses).
 * The kernels have no profile id of their own: stage 1 is charged to k_spatial, the weighted stage 2 to k_weights, the
 * counting stage 2 and the mean over the lattices to k_finalize.  Asynchronous on `stream` like vet_spatial_entropy. */
int vet_user_entropy(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                     double *d_entropy, double *d_weights, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_user_entropy_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                         double *d_entropy, double *d_weights, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_user_entropy_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                          int window, int stride, double *h_entropy, double *h_weights, int32_t *h_samples);

/* ---- pairwise viewer divergence: a U x U Jensen-Shannon matrix per row --------------------------------
 * The question that needs two histograms: do viewers look at the same places?  Rows are vet_user_entropy's: window = w,
 * stride = s, R = vet_window_rows(T, w, s), row r covers frames [r*s, r*s + w).  For a lattice of n tiles let h_u be viewer u's
 * histogram of the row — exactly what vet_user_entropy returns in d_weights for that lattice: the exact FP64 weight rows added
 * in ascending frame order (weighted Fibonacci lattices), counts (unweighted and binned lattices) — W_u the sum over its keys and
 *   S(h) = -sum_keys (h_t / W) log2(h_t / W)
 * the reference's `entropy` of compute_spatial_entropy / compute_naive_spatial_entropy BEFORE it is divided by the normaliser
 * (utilities/entropy_utils.py:194-198, :425-440; unnormalised bits on purpose: the unweighted normaliser depends on the sample
 * count and differs between the three terms).  Then
 *   D_k(u, v) = S(h_u + h_v) - (W_u S(h_u) + W_v S(h_v)) / (W_u + W_v)
 *   D(u, v)   = mean over the plan's lattices of D_k(u, v)            bits, 0 <= D <= H2(W_u / (W_u + W_v)) <= 1
 * S(h_u + h_v) is the reference's entropy of ONE dict holding both viewers' samples of the row: D is the Jensen-Shannon
 * divergence with each viewer weighted by their mass.
 *   D(u, v) is NaN when either viewer has no sample in the row (d_samples 0, d_status[1] += 1 per such (row, viewer)); such
 *     rows are data, not errors, as in vet_user_entropy: the _host entry never returns VET_ERR_EMPTY;
 *   D(u, v) is NaN exactly where one of the reference's three entropies is: a key whose sum is 0.0, or whose h_t / W underflows
 *     to 0 (0 * log2 0);
 *   D(u, u) is +0.0 for a present viewer (NaN where the viewer's own S is); the matrix is symmetric bit for bit.
 *   d_div     [R][U][U]
 *   d_samples [U][R]   the viewer's present samples of the row, as vet_user_entropy                             (nullable)
 *   d_status  [2]      {bad, #(row, viewer) without a sample}; the call ADDS, the caller zeroes               (nullable)
 * Three stages, the rows in chunks (as many rows as fit 256 MB of histograms, at least one), so the workspace is bounded
 * whatever R is; everything lives in the context's grow-only workspace, no allocation in steady state:
 *   1 k_user_dirs (vet_user_entropy's, unchanged): direction ids transposed once, [U][T] i32;
 *   2 per lattice and chunk: every viewer's histogram [rows][U][n] f64 — k_user_hist_w runs k_user_entropy_w's walk (the same
 *     add_exact_rows / waves_in_order sequence and wave split, so h_u has d_weights' bits), k_user_hist_c counts with
 *     k_user_entropy_c's walk — with W_u and a flag: no sample, or the viewer's own S is NaN under the reference's q * log2 q;
 *   3 k_user_divergence, the pair stage, in the overlap form.  With f(x) = x log2 x, W S(h) = f(W) - sum_t f(h_t), so
 *       D_k = ( f(W_u + W_v) - (f(W_u) + f(W_v)) - sum_t [ f(a_t + b_t) - (f(a_t) + f(b_t)) ] ) / (W_u + W_v)
 *     and the bracket is zero unless both viewers have weight on tile t: one FP64 log2 per tile of the OVERLAP of the two
 *     supports per pair.  A workgroup owns a 32 x 32 block of pairs of one row, upper triangle only, stages the two groups of
 *     histograms through LDS 32 tiles at a time and walks the tiles in ascending order with one accumulator per pair; the
 *     lower triangle is a copy.  The pooled term's NaN: a tile with 0 < a_t + b_t < (W_u + W_v) * 2^-1000 takes a slow path
 *     that performs the reference's division and marks the pair where the quotient is 0.
 *   Several lattices: lattice 0's pair stage stores D_0 / K, lattice k's adds D_k / K, in lattice order, for every pair alike.
 * D(u, v) is a pure function of the plan, the window and the two viewers' own samples of the row: the same bits whatever
 * stride selected the row, wherever its frames lie in the call, whichever other viewers the call holds, however the rows are
 * chunked, from run to run, and between the ids and the grid entry points.
 * VET_ERR_INVALID: as vet_user_entropy.  VET_ERR_UNSUPPORTED (checked before anything is launched or allocated):
 * vet_user_entropy's limits (n * 4 bytes of LDS for a counting lattice, n * 8 for a weighted one, whose exact rows must be on
 * the device; U * R < 2^31; n_frames <= 65535 * 64) and fewer than 2^31 blocks of 32 x 32 pairs (U < 2 097 120).
 * Profile ids: stage 1 is charged to k_spatial, the histograms as vet_user_entropy's (k_weights / k_finalize), the pair stage to
 * k_finalize.  Asynchronous on `stream` like vet_spatial_entropy. */
int vet_user_divergence(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                        double *d_div, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_user_divergence_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                            double *d_div, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_user_divergence_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                             int n_frames, int window, int stride, double *h_div, int32_t *h_samples);

/* ---- window-to-window attention divergence: a lag band of Jensen-Shannon distances -------------------
 * The question a windowed entropy series cannot answer: WHEN does the audience's attention move?  A crowd that jumps from one
 * side of the sphere to the other keeps its entropy; the distance between the pooled histogram of one window and that of a
 * later one shows the jump.  Rows are vet_spatial_entropy_windowed's: window = w, stride = s, R = vet_window_rows(T, w, s), row r
 * covers frames [r*s, r*s + w).  For a lattice of n tiles let P_r be the pooled histogram of row r — exactly what
 * vet_spatial_entropy_windowed returns in d_weights for that lattice: `dtable`'s FP64 frame sums added in ascending frame order
 * (weighted Fibonacci lattices), counts (unweighted and binned lattices) — W_r the sum over its keys and
 *   S(h) = -sum_keys (h_t / W) log2(h_t / W)
 * the reference's `entropy` of compute_spatial_entropy / compute_naive_spatial_entropy BEFORE it is divided by the normaliser
 * (utilities/entropy_utils.py:194-198, :425-440).  For the lags l = 1 .. L, L = max_lag (in rows):
 *   D_k(r, l) = S(P_r + P_{r+l}) - (W_r S(P_r) + W_{r+l} S(P_{r+l})) / (W_r + W_{r+l})
 *   D(r, l)   = mean over the plan's lattices of D_k(r, l)       bits, 0 <= D <= H2(W_r / (W_r + W_{r+l})) <= 1
 * S(P_r + P_{r+l}) is the reference's entropy of ONE dict holding the samples of both windows (overlapping windows, s*l < w,
 * hold the shared frames twice): D is the Jensen-Shannon divergence with each window weighted by its mass; 0 = the same tiles
 * in the same proportions, H2 of the mass split (1 for equal masses) = disjoint tiles.  Lag 1 is the per-segment "attention
 * shift" series, L = R - 1 the upper triangle of the video's recurrence matrix.
 *   d_div     [R][L]   d_div[r][l - 1] = D(r, l); NaN where r + l >= R (there is no such row), where either window has no
 *                      sample (such rows are data, not errors: the _host entry never returns VET_ERR_EMPTY), and exactly
 *                      where one of the reference's three entropies is NaN: a key whose sum is 0.0, or whose h_t / W
 *                      underflows to 0 (0 * log2 0)
 *   d_samples [R]      present samples per row, as vet_spatial_entropy_windowed                                 (nullable)
 *   d_status  [2]      {bad, #rows without a sample}; the call ADDS, the caller zeroes                          (nullable)
 * Three stages; everything lives in the context's grow-only workspace, no allocation in steady state:
 *   1 vet_spatial_entropy_windowed's stage 1, unchanged: every frame's histogram once (k_weights_gather / k_window_tiles);
 *   2 per lattice and chunk of pair rows (as many as fit 256 MB of histograms together with the halo of L rows their lags
 *     reach, at least one): the row histograms [rows][n] f64 — k_window_hist_w runs k_window_entropy_w's sum (the same
 *     additions in ascending frame order, so P_r has d_weights' bits up to the sign of zero), k_window_hist_c counts — with W_r
 *     and a flag: no sample, or the row's own S is NaN under the reference's q * log2 q;
 *   3 k_window_divergence, the pair stage, in vet_user_divergence's overlap form: with f(x) = x log2 x,
 *       D_k = ( f(W_a + W_b) - (f(W_a) + f(W_b)) - sum_t [ f(a_t + b_t) - (f(a_t) + f(b_t)) ] ) / (W_a + W_b)
 *     one FP64 log2 per tile on which both windows have weight.  One thread owns one pair (r, l) and walks the tiles in
 *     ascending order; a workgroup takes RB rows x LB lags — (256, 1) for max_lag = 1, (32, 8) up to 8, (8, 32) beyond, chosen
 *     from max_lag alone — and stages the RB + (RB + LB - 1) histograms it needs through LDS.  The pooled term's NaN: a tile
 *     with 0 < a_t + b_t < (W_a + W_b) * 2^-1000 takes a slow path that performs the reference's division and marks the pair
 *     where the quotient is 0.
 *   Several lattices: lattice 0's pair stage stores D_0 / K, lattice k's adds D_k / K, in lattice order, for every pair alike.
 * D(r, l) is a pure function of the plan, the window and the frames of rows r and r + l: the same bits whatever n_frames,
 * stride and max_lag selected the pair, wherever it falls in a launch or a row chunk, whichever block shape ran it, from run to
 * run, and between the ids and the grid entry points.
 * VET_ERR_INVALID (before anything is launched or allocated): vet_spatial_entropy_windowed's, R < 2, max_lag < 1 or
 * max_lag > R - 1.  VET_ERR_UNSUPPORTED (likewise): vet_spatial_entropy_windowed's limits (n * 4 bytes of LDS for a counting
 * lattice, n * 8 for a weighted one, whose exact rows must be on the device), max_lag > 65535 lag blocks, R >= 2^31 - 256.
 * Profile ids: stage 1 as vet_spatial_entropy_windowed's (k_weights / k_spatial), stage 2 to k_finalize, the pair stage to
 * k_transition — the one id the call does not use otherwise, so that the three stages can be told apart.  Asynchronous on
 * `stream` like vet_spatial_entropy. */
int vet_window_divergence(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                          int max_lag, double *d_div, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_window_divergence_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int max_lag,
                              double *d_div, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_window_divergence_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                               int n_frames, int window, int stride, int max_lag, double *h_div, int32_t *h_samples);

/* ---- attention coverage: the top-k tile sets of a window and how well they forecast later windows ------
 * How many tiles hold 80 % / 95 % of the audience's attention in a segment, which tiles are they, and what share of the attention
 * of the NEXT segments do they still hold (tile-based delivery: fetch these tiles in high quality)?  Rows are
 * vet_spatial_entropy_windowed's: window = w, stride = s, R = vet_window_rows(T, w, s), row r covers frames [r*s, r*s + w).
 * Only LATTICE 0 takes part — the lattice whose tile_weights every row call returns; a plan of several lattices gives the bits
 * of the plan of its first.  Let h_r[t] >= 0 be row r's histogram over lattice 0's n tiles: the windowed call's d_weights bit for
 * bit, taken by absolute value (a key whose weight underflowed to 0.0 carries no mass).  Inputs: `fractions`, a HOST array of
 * 1 <= Q <= 8 values, each in (0, 1], strictly increasing; max_lag = L in rows, 0 <= L <= R - 1.
 *   rank order   order_r[j] = the tile at rank j: weight descending, equal weights by tile index ascending.  All n tiles are
 *                listed, so the tiles of weight 0 come last in index order.  rank_r[t] = the rank of tile t.
 *   mass         C_0 = 0, C_j = C_{j-1} + h_r[order_r[j-1]]: ONE accumulator, one FP64 addition per tile, in rank order (numpy's
 *                cumsum of the sorted weights); W_r = C_n.  The summation order is part of the contract: with it `tiles` is an
 *                exact integer statement.
 *   d_tiles   i32 [R][Q]        tiles[r][i] = the smallest k with C_k >= fractions[i] * W_r (the product is one IEEE multiply);
 *                               0 where W_r = 0: a row without a sample, or a weighted plan none of whose tiles is inside any
 *                               viewport's FoV
 *   d_hit     f64 [R][L+1][Q]   hit[r][l][i] = sum over {t : rank_r[t] < tiles[r][i]} of h_{r+l}[t], divided by W'_{r+l}, the
 *                               windowed call's row total (the keys' values added in lane order, wave_sum's butterfly; counts:
 *                               the row's samples).  l = 0: the coverage actually reached, >= fractions[i] up to rounding;
 *                               l >= 1: the share of row r + l's attention that row r's tile set still holds.  NaN where
 *                               r + l >= R, where W_r = 0 and where W'_{r+l} = 0 — data, not an error.  The sum runs in one
 *                               wave: lane j adds its tiles j, j + 64, ... in ascending order, then wave_sum's butterfly — a
 *                               function of n alone
 *   d_order   i32 [R][n]        order_r                                                                             (nullable)
 *   d_samples i32 [R]           present samples per row, as vet_spatial_entropy_windowed                            (nullable)
 *   d_status  [2]               {bad, #rows without a sample}; the call ADDS, the caller zeroes                     (nullable)
 * tiles[r], order_r and hit[r][0] are pure functions of the plan, the window, row r's frames and (per column i) fractions[i];
 * hit[r][l][i] depends on row r + l's frames besides.  None depends on stride, max_lag, the other fractions, n_frames, the row
 * chunk or the entry point: the same bits.
 * Four stages, everything in the context's grow-only workspace: 1 vet_spatial_entropy_windowed's stage 1; 2 per chunk of rows
 * (as many as fit 256 MB of histograms together with the halo of L rows, at least one) lattice 0's row histograms, as
 * vet_window_divergence's stage 2; 3 k_coverage_rank, one workgroup per row: (weight bits, tile) records sorted in LDS (bitonic,
 * padded to a power of two with records that sort last), the running sum by one lane, the Q thresholds, every tile's rank; 4
 * k_coverage_hits, one wave per (row, lag).
 * VET_ERR_INVALID (before anything is launched or allocated): vet_spatial_entropy_windowed's, fractions NULL, not strictly
 * increasing or outside (0, 1], Q < 1 or Q > 8, max_lag < 0 or max_lag > R - 1.  VET_ERR_UNSUPPORTED (likewise): a lattice 0 of
 * more than 2048 tiles (the LDS sort holds 2048 records of 16 bytes: every Fibonacci lattice the other calls accept and the naive
 * 10 x 20 degree cells fit, 1 x 1 degree cells do not), max_lag >= 65535 * 16, R >= 2^31 - 256, and
 * vet_spatial_entropy_windowed's limits.
 * Profile ids: stage 1 as vet_spatial_entropy_windowed's (k_weights / k_spatial), stage 2 to k_finalize, k_coverage_rank to
 * k_transition and k_coverage_hits to k_wtab — ids the call does not use otherwise, so that the stages can be told apart.
 * Asynchronous on `stream` like vet_spatial_entropy. */
int vet_coverage(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                 int max_lag, const double *fractions, int n_fractions, int32_t *d_tiles, double *d_hit, int32_t *d_order,
                 int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_coverage_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int max_lag,
                     const double *fractions, int n_fractions, int32_t *d_tiles, double *d_hit, int32_t *d_order,
                     int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa; h_order
 * and h_samples may be NULL. */
int vet_coverage_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                      int window, int stride, int max_lag, const double *fractions, int n_fractions, int32_t *h_tiles,
                      double *h_hit, int32_t *h_order, int32_t *h_samples);

/* ---- viewer-to-crowd divergence: each viewer's Kullback-Leibler divergence from the pooled crowd ------
 * How typical is each viewer of the audience, window by window, and how much of a window's pooled entropy is disagreement between
 * viewers rather than each viewer looking around?  Rows are vet_user_entropy's and vet_spatial_entropy_windowed's: window = w,
 * stride = s, R = vet_window_rows(T, w, s), row r covers frames [r*s, r*s + w).  For a lattice of n tiles let h_u be viewer u's
 * histogram of the row with total W_u — exactly what vet_user_entropy returns in d_weights — P_r the row's pooled histogram with
 * total W_r — exactly what vet_spatial_entropy_windowed returns in d_weights — and
 *   S(h) = -sum_keys (h_t / W) log2(h_t / W)
 * the reference's `entropy` of compute_spatial_entropy / compute_naive_spatial_entropy BEFORE it is divided by the normaliser
 * (utilities/entropy_utils.py:194-198, :425-440).  Then
 *   D_k(u, r)  = sum_{t in keys of h_u} q_t log2(q_t / p_t),   q_t = h_ut / W_u,   p_t = P_rt / W_r
 *   D(u, r)    = mean over the plan's lattices of D_k(u, r)     bits, 0 <= D <= log2(W_r / W_u)
 * 0 = the viewer looks where the crowd looks, in the crowd's proportions; log2(W_r / W_u) = the viewer shares no tile with
 * anybody.  Per row, summed over the viewers with a sample in it,
 *   pooled[r]  = S(P_r)
 *   within[r]  = sum_u (W_u / W_r) S(h_u)
 *   between[r] = sum_u (W_u / W_r) D_k(u, r)        (taken directly, not as a difference)
 * each the mean over the lattices; pooled = within + between up to rounding: between is the generalised Jensen-Shannon
 * divergence of the whole audience.
 *   d_div     [U][R]   user-major like vet_user_entropy.  NaN where the viewer has no sample in the row (such slots are data, not
 *                      errors: the _host entry never returns VET_ERR_EMPTY), where the viewer's own S is NaN under the
 *                      reference's q * log2 q (a key whose sum is 0.0, or whose h_t / W underflows to 0), and where the row's
 *                      own S is
 *   d_rows    [3][R]   pooled, within, between.  pooled is NaN exactly where the row has no sample or its own S is NaN; within
 *                      and between are NaN there and where any present viewer's own S is NaN                     (nullable)
 *   d_samples [U][R]   present samples per (viewer, row), as vet_user_entropy                                   (nullable)
 *   d_status  [2]      {bad, #(row, viewer) slots without a sample}; the call ADDS, the caller zeroes             (nullable)
 * Stages; everything lives in the context's grow-only workspace, no allocation in steady state:
 *   1 k_user_dirs, unchanged: direction ids transposed once;
 *   2 vet_spatial_entropy_windowed's stage 1, unchanged: every frame's histogram once;
 *   3 per lattice and chunk of rows (as many as fit 256 MB of pooled histograms, their log2 tables and per-viewer statistics,
 *     at least one): k_window_hist_w/_c leave P[rows][n], W_r and the row's flag, k_crowd_logp log2 p_t per row and tile;
 *   4 k_crowd_w (weighted Fibonacci lattices) / k_crowd_c (unweighted and binned lattices): one workgroup per (row, viewer),
 *     the viewer fastest.  The viewer's histogram is built in LDS by vet_user_entropy's walk (the same wave split, the same
 *     order of additions) and never written to memory; one wave takes W_u, S(h_u) and D = sum q_t (log2 q_t - log2 p_t)
 *     against the row's log2 p table read from global memory — the one FP64 log2 per key tile serves S and D — every
 *     reduction in lane order followed by the wave butterfly;
 *   5 k_crowd_rows: one wave per row, each lane sums its viewers in ascending order.
 *   Several lattices: lattice 0 stores its value / K, lattice k adds its own, in lattice order.
 * A value is a pure function of the plan, the window and the frames of its row: the same bits whatever n_frames and stride
 * selected the row, wherever it falls in a launch or a row chunk, from run to run, and between the ids and the grid entry points.
 * VET_ERR_INVALID (before anything is launched or allocated): vet_user_entropy's.  VET_ERR_UNSUPPORTED (likewise):
 * R * n_users >= 2^31, n_frames > 65535 * 64, vet_user_entropy's and vet_spatial_entropy_windowed's limits on the plan.
 * Profile ids: k_user_dirs to k_spatial, stage 2 as vet_spatial_entropy_windowed's (k_weights / k_spatial), k_window_hist_* and
 * k_crowd_rows to k_finalize, k_crowd_w / k_crowd_c to k_transition — the one id the call does not use otherwise, so that the
 * (row, viewer) stage can be told from stage 2's gather.  Asynchronous on `stream` like vet_spatial_entropy. */
int vet_crowd_divergence(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                         double *d_div, double *d_rows, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_crowd_divergence_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                             double *d_div, double *d_rows, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa; h_rows and
 * h_samples may be NULL. */
int vet_crowd_divergence_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                              int n_frames, int window, int stride, double *h_div, double *h_rows, int32_t *h_samples);

/* ---- bootstrap confidence bands over viewers for per-frame and windowed entropy ----------------------
 * Every entropy the engine reports is a point estimate from one sample of viewers; an entropy from 30 viewers and one from 300
 * are not comparable without an interval.  Viewers are the independent unit, so the audience is resampled with replacement (the
 * cluster bootstrap) and the series recomputed, B times in one call.
 * - Rows.  Rows are vet_spatial_entropy_windowed's.  Row r covers frames [r*stride, r*stride + window).  window = 1, stride = 1 is
 *   the per-frame series.
 * - Draw.  For replicate b (0-based) and draw j = 0 ... U-1, all in unsigned 64-bit arithmetic mod 2^64:
 *     z = seed + (b*U + j + 1) * 0x9E3779B97F4A7C15
 *     z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     viewer = ((z >> 32) * U) >> 32
 *   c[b][u] = the number of draws of replicate b that picked u, and sum_u c[b][u] = U.  Replicate b does not depend on B.  The same
 *   resample applies to every row and every lattice of a call.  This is the cluster bootstrap: a viewer's whole trajectory stays
 *   together.
 * - Value.  rep[r][b] is the reference's compute_spatial_entropy on ONE dict (naive plans use compute_naive_spatial_entropy).  The
 *   dict holds every present sample of the row's frames for every drawn viewer, frame-major, then in draw order.  A viewer drawn c
 *   times is entered c times.  The value is per lattice, then the mean over the lattices, as compute_entropy takes it.  The
 *   normaliser follows the replicate's own total.  A replicate whose drawn viewers have no sample in the row is NaN.  That is
 *   data, not an error.  Whatever the reference's 0 * log2 0 makes NaN is NaN: a key tile whose replicate sum is 0.0, or whose q
 *   underflows to 0.
 * - Summary per row.  Taken over the m finite replicates, sorted ascending: mean; sd: two-pass, ddof = 1, NaN for m < 2; lo and hi:
 *   the quantiles (1 - confidence)/2 and 1 - (1 - confidence)/2, by linear interpolation between order statistics at position
 *   q*(m - 1): x[i] + (x[i+1] - x[i])*g; valid = m.  m = 0 gives NaN for all four.
 * - Bits.  A replicate's bits depend on the plan, the window, the row's frames, U, seed and b only.  They do not depend on stride,
 *   B, the number of rows, the row chunk or the entry point.
 *   d_summary    [4][R]      mean, sd, lo, hi
 *   d_replicates [R][B]      rep[r][b]                                                                          (nullable)
 *   d_weights    [R][B][n0]  lattice 0's replicate histograms sum_u c[b][u] h_u: PLAIN VALUES, +0.0 = no weight.  Not the dense
 *                            tile_weights encoding: a key whose value is 0.0 reads +0.0 like a tile that is no key (whether such
 *                            a key exists decides a NaN above, but is not recorded per tile)                       (nullable)
 *   d_valid      [R]         m, the finite replicates of the row                                                 (nullable)
 *   d_status     [2]         {bad, unused}; the call ADDS to [0], the caller zeroes                               (nullable)
 * For one row, replicate b's histogram is sum_u c[b][u] h_u with h_u viewer u's own row histogram (vet_user_entropy's d_weights):
 * a row's B replicate histograms are a [B x U] . [U x n] FP64 matrix product.  Stages; everything lives in the context's grow-only
 * workspace, no allocation in steady state:
 *   1 k_user_dirs, unchanged: direction ids transposed once;
 *   2 k_bootstrap_counts: c[B][U] u16 from the draw, integer atomics (exact in any order);
 *   3 per lattice and chunk of rows (as many as fit 256 MB of histograms, at least one): vet_user_divergence's k_user_hist_w/_c,
 *     unchanged, leave hist[rows][U][n] f64; k_bootstrap_zero_keys marks, for the flagged (row, viewer) slots of weighted lattices
 *     only, the tiles that are keys of the viewer with the value 0.0 (underflowing power_factor);
 *   4 k_bootstrap_gemm: one workgroup per (row, 16 replicates); each of its 4 waves runs the whole K loop over the viewers in
 *     ascending blocks of four into one accumulator per 16-tile column block with v_mfma_f64_16x16x4_f64 (no split-K, no atomics)
 *     and leaves the 16 x n block in LDS; then one wave per replicate takes W, S and the normaliser as vet_user_entropy does
 *     (counting lattices: log2(n) if W > n, else log2(W), as compute_spatial_entropy), every reduction in lane order followed by the
 *     wave butterfly.  Lattice 0 stores value / K, lattice k adds its own, in lattice order;
 *   5 k_bootstrap_summary: one workgroup per row sorts the finite replicates in LDS.
 * The summation order inside one 16x16x4 MFMA is the hardware's and fixed: replicates reproduce bit for bit; against the reference
 * they agree to rounding (the project's 1e-6 contract; integer plans exactly, their sums being integers).
 * VET_ERR_INVALID (before anything is staged, launched or allocated): vet_user_entropy's; replicates outside [1, 4096]; confidence
 * outside (0, 1).  VET_ERR_UNSUPPORTED (likewise): n_users > 65535 (16-bit counts); a lattice of more than 1276 tiles (the 16 x n
 * FP64 block must fit the 160 KB LDS); R * n_users >= 2^31, n_frames > 65535 * 64, vet_user_entropy's limits on the plan.
 * Profile ids: k_user_dirs to k_spatial, the histogram kernels as vet_user_entropy's (k_weights / k_finalize), k_bootstrap_gemm to
 * k_transition — the one id the call does not use otherwise —, the rest to k_finalize.  Asynchronous on `stream` like
 * vet_spatial_entropy. */
int vet_bootstrap_entropy(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                          int replicates, uint64_t seed, double confidence, double *d_summary, double *d_replicates,
                          double *d_weights, int32_t *d_valid, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_bootstrap_entropy_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                              int replicates, uint64_t seed, double confidence, double *d_summary, double *d_replicates,
                              double *d_weights, int32_t *d_valid, int32_t *d_status, void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa;
 * h_replicates, h_weights and h_valid may be NULL. */
int vet_bootstrap_entropy_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                               int n_frames, int window, int stride, int replicates, uint64_t seed, double confidence,
                               double *h_summary, double *h_replicates, double *h_weights, int32_t *h_valid);
/* The draw alone: runs k_bootstrap_counts on the plan's context and downloads c[replicates][n_users], so that the draw can be
 * pinned on its own.  Synchronous.  Errors as above (replicates, n_users). */
int vet_bootstrap_counts_host(vet_plan *plan, int n_users, int replicates, uint64_t seed, uint16_t *h_counts);

/* ---- two-audience permutation test of attention divergence -------------------------------------------
 * Headset against desktop, sound against mute, first viewing against second: do two groups of viewers look at different places,
 * in which segments, and by more than a random split of the same viewers would produce?  Viewers are the independent unit, so
 * the null distribution comes from relabelling viewers, P times in one call.
 * - Groups.  groups[U], int8, HOST memory in every entry, read and validated before the call returns: 0 = audience A, 1 = audience
 *   B, -1 = excluded.  U_A, U_B >= 1.  The included viewers in ascending viewer order are v_0 ... v_{N-1}, N = U_A + U_B.
 * - Rows.  Rows are vet_spatial_entropy_windowed's.  Row r covers frames [r*stride, r*stride + window).  window = n_frames is the
 *   single whole-video row.
 * - Statistic of one labelling, per lattice.  A = sum_{u in A} h_u and B = sum_{u in B} h_u, h_u viewer u's own row histogram
 *   (vet_user_entropy's d_weights), the viewers added in ascending order, in blocks of four, into one accumulator, exactly as
 *   k_bootstrap_gemm sums.  D_k = S(A + B) - (W_A*S(A) + W_B*S(B)) / (W_A + W_B), S(h) = -sum_keys (h_t / W) log2(h_t / W) and W as
 *   in vet_window_divergence; D = the mean over the lattices, in bits.  In reference terms: three compute_spatial_entropy calls
 *   (naive plans: compute_naive_spatial_entropy), on group A's present samples of the row, on group B's, and on a single dict
 *   holding both, each group entered frame-major, then by ascending viewer, A before B in the pooled dict.  D is NaN where either
 *   group has no sample in the row.  That is data, not an error.  D is NaN exactly where one of the reference's three entropies is:
 *   a key whose sum is 0.0 (the bootstrap's zero-key rule, applied to the members of each group and to all included viewers for
 *   the pooled term), or a proportion that underflows to 0.  B is never computed as pooled - A: the subtraction would leave
 *   rounding residue on tiles that are exactly 0, and a tile is a key iff its sum is > 0.
 * - Labellings.  Labelling 0 is the observed `groups`; labellings 1 ... P are permutations, P = permutations in [1, 4096].  For
 *   permutation b (0-based) and included index i, all in unsigned 64-bit arithmetic mod 2^64:
 *     z = seed + (b*N + i + 1) * 0x9E3779B97F4A7C15
 *     z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *     key = (z >> 16 << 16) | i
 *   The U_A included viewers with the smallest keys are audience A, the rest B; excluded viewers stay excluded.  Permutation b does
 *   not depend on P.  One permutation serves every row and every lattice: a viewer's trajectory stays together.  N <= 16384 (one
 *   permutation's keys are ranked in LDS).
 * - Summary per row, over the m finite values of the row's P permutation statistics: observed = D of labelling 0;
 *   p_value = (1 + #{finite null >= observed}) / (1 + m); null_mean; null_crit = the quantile `confidence` by the bootstrap's rule
 *   (linear interpolation between order statistics at position q*(m - 1)); valid = m; p_adjusted, the max-statistic family-wise
 *   correction over the rows of the call: maxnull[b] = the largest finite null value of permutation b over all rows, M = the
 *   permutations that have one, p_adjusted[r] = (1 + #{b: maxnull[b] >= observed[r]}) / (1 + M).  observed NaN: p_value and
 *   p_adjusted NaN.  m = 0: null_mean and null_crit NaN.
 * - Ties.  >= is taken on the stored doubles.  Labelling 0 goes through the same kernel and the same operand order as the
 *   permutations: a permutation that reproduces the observed partition reproduces its bits, so ties are exact.
 * - Bits.  A labelling's D depends on the plan, the window, the row's frames and the labelling's two viewer sets only.  It does
 *   not depend on P, stride, the number of rows, the row chunk or the entry point.
 *   d_summary [5][R]      observed, p_value, p_adjusted, null_mean, null_crit
 *   d_null    [R][P]      the permutation statistics                                                              (nullable)
 *   d_weights [R][2][n0]  lattice 0's histograms of the observed A and B: PLAIN VALUES, +0.0 = no weight        (nullable)
 *   d_samples [2][R]      the present samples of the observed A and B in the row                                 (nullable)
 *   d_valid   [R]         m                                                                                       (nullable)
 *   d_status  [2]         {bad, unused}; the call ADDS to [0], the caller zeroes                                  (nullable)
 * Stages; everything lives in the context's grow-only workspace, no allocation in steady state:
 *   1 k_user_dirs, unchanged;
 *   2 k_group_labels: one workgroup per permutation computes the keys, sorts them in LDS (bitonic) and writes labels[P+1][U] u8
 *     (0, 1, 255 = excluded), row 0 the observed groups; no atomics;
 *   3 per lattice and chunk of rows (as many as fit 256 MB of histograms, at least one): k_user_hist_w/_c, unchanged, with the
 *     per-(viewer, row) samples; on weighted lattices k_bootstrap_zero_keys, unchanged;
 *   4 k_group_gemm: one workgroup per (row, 8 labellings), 4 waves.  Rows 0-7 of the 16 x 16 x 4 FP64 MFMA tile hold the A sums of
 *     the eight labellings, rows 8-15 their B sums: the A operand is labels == 0 for i < 8 and labels == 1 for i >= 8, the B
 *     operand hist[u][t] is loaded once and serves both.  K loop as k_bootstrap_gemm: ascending blocks of four viewers, one
 *     accumulator per column block, no split-K, no atomics.  The 16 x n block stays in LDS; then per labelling W and S over A,
 *     over B and over a_t + b_t, the zero-key rule, D_k.  Lattice 0 stores D_0 / K, lattice k adds its own, in lattice order.
 *     Speed only, no effect on a value: the edges are predicated through the mask operand (loads without branches), the kernel
 *     asks for a two-waves-per-SIMD register budget (accumulators stay in VGPRs), and the one-dimensional launch is remapped so
 *     that the workgroups of one row share an XCD's L2;
 *   5 k_group_samples; k_group_maxnull: one thread per permutation walks the rows of null[R][P]; k_group_summary: one workgroup per
 *     row takes the counts, the mean and sorts the finite values in LDS for the quantile.
 * VET_ERR_INVALID (before anything is staged, launched or allocated): the windowed calls'; a group value outside {-1, 0, 1}; an
 * empty group; permutations outside [1, 4096]; confidence outside (0, 1).  VET_ERR_UNSUPPORTED (likewise): N > 16384; a lattice of
 * more than 1276 tiles (the 16 x n FP64 block must fit the 160 KB LDS); R * n_users >= 2^31, n_frames > 65535 * 64,
 * vet_user_entropy's limits on the plan.  Profile ids: as the bootstrap's, k_group_gemm to k_transition, k_group_labels and stage
 * 5 to k_finalize.  Asynchronous on `stream` like vet_spatial_entropy (`groups` is consumed before the call returns). */
int vet_group_divergence(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                         const int8_t *groups, int permutations, uint64_t seed, double confidence, double *d_summary,
                         double *d_null, double *d_weights, int32_t *d_samples, int32_t *d_valid, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_group_divergence_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                             const int8_t *groups, int permutations, uint64_t seed, double confidence, double *d_summary,
                             double *d_null, double *d_weights, int32_t *d_samples, int32_t *d_valid, int32_t *d_status,
                             void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa; h_null,
 * h_weights, h_samples and h_valid may be NULL. */
int vet_group_divergence_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                              int n_frames, int window, int stride, const int8_t *groups, int permutations, uint64_t seed,
                              double confidence, double *h_summary, double *h_null, double *h_weights, int32_t *h_samples,
                              int32_t *h_valid);
/* The draw alone: runs k_group_labels on the plan's context and downloads labels[permutations + 1][n_users] (0 = A, 1 = B, 255 =
 * excluded; row 0 the observed groups), so that the draw can be pinned on its own.  Synchronous.  Errors as above (groups,
 * permutations, N). */
int vet_group_labels_host(vet_plan *plan, int n_users, const int8_t *groups, int permutations, uint64_t seed, uint8_t *h_labels);

/* ---- sliding-window transition entropy: the transitions of a window of frame pairs pooled ----------
 * A video of T frames has P = T - 1 frame pairs; pair f is (frame f, frame f + 1).  For 1 <= window <= P and stride >= 1
 * there are R = vet_window_rows(P, window, stride) rows; row r covers pairs [r*stride, r*stride + window).  Row r is, for
 * every lattice of the plan, what compute_transition_entropy (utilities/entropy_utils.py:213-332) returns when BOTH dicts hold
 * one entry per (pair, user) of the window — keys unique per (pair, user), inserted pair-major then in user order, the prior
 * dict holding the direction at frame f and the current dict the direction at frame f + 1, and only the (pair, user)
 * entries present in both frames inserted — then the mean over the lattices as TransitionEntropyAnalyzer.compute_entropy
 * takes it.  In the reduced form the kernels evaluate (above) it is the per-pair algorithm with "user index" replaced by
 * the sample's rank in the pooled order: per source tile m, K = 1 + #distinct destinations after the first sample, w = the
 * count of the bucket whose first appearance is latest, cell = -(m/N) K (w/m) log2(w/m); the normaliser is log2(n) if
 * N > n, else log2(N), N = pooled samples.  Quirks are reproduced: N = 1 gives the reference's NaN (0 / 0).
 *   A window without a common sample: NaN in d_entropy, 0 in d_samples and d_status[1] += 1 — what vet_transition_entropy
 *   does with such a pair; the _host entry then returns VET_ERR_EMPTY (outputs are still written).
 * window = 1, stride = 1 is the per-pair series (d_samples = vet_transition_entropy's d_common).
 *   d_entropy  [R]
 *   d_srccount [R*n_0]  lattice 0's pooled samples per source tile (the reference's weight_per_tile)   (nullable)
 *   d_samples  [R]      N of the row                                                                  (nullable)
 *   d_status   [2]      {bad, #rows without a common sample}; the call ADDS, the caller zeroes        (nullable)
 * The per-sample pairs are not returned; vet_transition_entropy has them.
 * Two stages per lattice.  1: k_window_tiles over all T frames — every sample is quantised and looked up once, whatever the
 * overlap — into [T][U] i32 of the context's grow-only workspace (one lattice's array, reused lattice after lattice; no
 * allocation in steady state).  2: k_window_transition — a row's pooled samples are a contiguous slice of that array
 * (sample q: source tiles[f0*U + q], destination tiles[f0*U + q + U], f0 = r*stride), walked by k_transition_big's row
 * algorithm (shared device code).  Every row is computed from scratch: first-appearance order makes the statistic
 * non-decomposable over frames, there is no running add / subtract.
 * A row is a pure function of the plan and of the samples of its window + 1 frames: integer atomics only, the FP64 cell sum
 * in a fixed order, the workgroup shape chosen by window * n_users alone — the same bits whatever stride selected the row,
 * wherever its frames lie in the call, from run to run, and between the grid and the ids entry points.
 * VET_ERR_INVALID: window < 1, stride < 1, window > n_frames - 1, n_frames < 2 (and what vet_transition_entropy refuses).
 * VET_ERR_UNSUPPORTED (checked before anything is launched or allocated): window * n_users >= 2^19 (the kernel packs
 * sample << 13 | hash slot), a lattice of more than 2800 tiles (TRANS_BIG_MAX_TILES).
 * Profile ids: stage 1 is charged to k_spatial (k_window_tiles, as above), stage 2 to k_transition, the mean over the
 * lattices to k_finalize.  Asynchronous on `stream` like vet_transition_entropy. */
int vet_transition_entropy_windowed(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames,
                                    int window, int stride, double *d_entropy, int32_t *d_srccount, int32_t *d_samples,
                                    int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_transition_entropy_windowed_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window,
                                        int stride, double *d_entropy, int32_t *d_srccount, int32_t *d_samples,
                                        int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE / VET_ERR_EMPTY when the status words are non-zero (outputs are
 * still written).  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_transition_entropy_windowed_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids,
                                         int n_users, int n_frames, int window, int stride, double *h_entropy,
                                         int32_t *h_srccount, int32_t *h_samples);

/* ---- per-viewer transition entropy: each user's own tile moves over time --------------------------
 * The transposed question of the windowed call: how predictably ONE viewer moves between tiles.  A video of T frames has
 * P = T - 1 frame pairs; pair f is (frame f, frame f + 1).  For 1 <= window <= P and stride >= 1 every user has
 * R = vet_window_rows(P, window, stride) rows; row (u, r) covers pairs [r*stride, r*stride + window) of user u and is, for
 * every lattice of the plan, what compute_transition_entropy (utilities/entropy_utils.py:213-332) returns when BOTH dicts hold
 * one entry per pair f of the row in which user u is present in frame f AND in frame f + 1 — keys unique per pair, inserted
 * in ascending pair order, the prior dict holding the direction at frame f and the current dict the direction at frame f + 1
 * — then the mean over the lattices as TransitionEntropyAnalyzer.compute_entropy takes it.  In the reduced form the kernels
 * evaluate (the windowed section above) "user index" is the pair's rank in the row.  Quirks are reproduced: N = 1 gives the
 * reference's NaN (0 / 0), so every window = 1 row is NaN or empty.
 *   a row without a common sample: NaN in d_entropy, 0 in d_samples and d_status[1] += 1.  Viewers join and leave, so such
 *     rows are data, not errors: the _host entry does NOT turn them into VET_ERR_EMPTY (vet_user_entropy's rule).
 * window = n_frames - 1 is the whole video (R = 1).  Outputs are user-major:
 *   d_entropy  [U][R]
 *   d_srccount [U][R][n_0]  lattice 0's samples per source tile                                           (nullable)
 *   d_samples  [U][R]       N of the row                                                                  (nullable)
 *   d_status   [2]          {bad, #rows without a common sample}; the call ADDS, the caller zeroes        (nullable)
 * Two stages:
 *   1 k_user_dirs (vet_user_entropy's, unchanged): every sample quantised once, its direction id written transposed, [U][T]
 *     i32, in the context's grow-only workspace (no allocation in steady state); the only place d_status[0] is raised.  One
 *     transposition serves every lattice: stage 2 looks up nearest[id];
 *   2 per (user, row) and lattice over the contiguous slice of the user's ids: pair q has the source nearest[dirs[u][f0 + q]]
 *     and the destination nearest[dirs[u][f0 + q + 1]], f0 = r*stride.
 *     window <= 64 (k_user_transition_wave): a row lives in one wave's registers, lane = pair, floor(64 / window) rows of one
 *       user per wave as segments; three walks of `window` cross-lane reads give every lane whether it is its source tile's
 *       first sample, m, whether it is its bucket's first sample and the bucket's count, then the tile's K and w, then the sum
 *       of the segment's cells in ascending lane order.  No LDS, no per-tile words, no atomics: the cost does not depend on
 *       the lattice size;
 *     window > 64 (k_user_transition): k_window_transition's body — k_transition_big's row algorithm, device code shared —
 *       with the destination at offset 1; 64 threads and 512 hash slots up to 256 pairs, 256 and 2048 up to 1024, 256 and
 *       4096 up to 2048 (packed pairs in LDS), else 1024 threads, 8192 slots, passes by the bucket bound 0.6 * 8192 - n and
 *       the packed pairs in per-workgroup global slices; persistent workgroups over the U * R rows.
 *     vet_test_user_transition_hash sends the short windows through the second kernel; the two agree to rounding.
 * A row is a pure function of the plan, `window` and its own window + 1 frames of its own user — which kernel runs and how
 * the wave is segmented included: the same bits whatever stride selected it, wherever its frames lie in the call, whichever
 * other users the call holds, from run to run, and between the ids and the grid entry points.
 * VET_ERR_INVALID: window < 1, stride < 1, window > n_frames - 1, n_frames < 2 (and what vet_transition_entropy_windowed
 * refuses about the plan).  VET_ERR_UNSUPPORTED (checked before anything is launched or allocated, for both stage-2 kernels
 * alike): a lattice of more than 2800 tiles (TRANS_BIG_MAX_TILES), window >= 2^19, U * R >= 2^31.
 * Profile ids: stage 1 is charged to k_spatial, stage 2 to k_transition, the mean over the lattices to k_finalize.
 * Asynchronous on `stream` like vet_transition_entropy. */
int vet_user_transition_entropy(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames,
                                int window, int stride, double *d_entropy, int32_t *d_srccount, int32_t *d_samples,
                                int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_user_transition_entropy_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                                    double *d_entropy, int32_t *d_srccount, int32_t *d_samples, int32_t *d_status,
                                    void *stream);
/* Host buffers ([n_frames][n_users] samples as everywhere): H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside
 * [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_user_transition_entropy_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids,
                                     int n_users, int n_frames, int window, int stride, double *h_entropy,
                                     int32_t *h_srccount, int32_t *h_samples);

/* ---- windowed Markov transition statistics: entropy rate, mutual information, the transition matrix ------
 * The three calls above evaluate the reference's compute_transition_entropy, whose value depends on first-appearance order (K, w).
 * These entries give the textbook quantities of the same tile-to-tile moves instead; they are plain functions of integer pair
 * counts and share nothing with that statistic but stage 1.
 * Parameters: window, stride and lag >= 1.  A video of T frames has T - lag pairs; pair f is (frame f, frame f + lag).  Row r
 * covers pairs [r*stride, r*stride + window), R = vet_window_rows(T - lag, window, stride) rows; window = T - lag is the whole
 * video's matrix (one row).  A (pair, user) is pooled when the user has a sample in both frames of the pair; the frames in
 * between do not matter.  Per lattice, with p / c the nearest tiles of the two samples (k_window_tiles' values):
 *   N pooled samples, n_pc samples per (source, destination), n_p = sum_c n_pc, m_c = sum_p n_pc, f(k) = k log2 k on integers
 *   (f(0) = f(1) = 0; log2 k from the context's table for k <= 4096, FP64 log2 beyond).  The five statistics, in bits but `stay`:
 *   0 rate        H(c | p) = (A - B) / N, A = sum_p f(n_p) and B = sum_pc f(n_pc) taken over the sources with at least two distinct
 *                 destinations ONLY: a source with one destination enters neither sum, so a row in which every source has one
 *                 destination is +0.0 exactly; any other source contributes at least 2 / N, so the value is never negative
 *   1 stationary  H(p) = log2 N - sum_p f(n_p) / N  (all sources)
 *   2 dest        H(c) = log2 N - sum_c f(m_c) / N
 *   3 mutual      dest - rate: the bits about the tile `lag` frames ahead that the tile now gives; not clamped, may sit within
 *                 rounding of 0
 *   4 stay        sum_p n_pp / N
 * each the mean over the plan's lattices (k_finalize over [K][5 R]).
 *   d_stats   [5][R]            statistic-major
 *   d_matrix  [R][n_0][n_0]     lattice 0's dense count matrix, source-major, i32                            (nullable)
 *   d_samples [R]               N of the row                                                                 (nullable)
 *   d_status  [2]               {bad, #rows without a pooled sample}; the call ADDS, the caller zeroes       (nullable)
 * A row with N = 0 has five NaN, samples 0 and a zero matrix: data, not an error (the _host entry returns VET_OK).  N = 1 is well
 * defined: rate, stationary, dest and mutual are 0, stay is 0 or 1.
 * Stage 1 is vet_transition_entropy_windowed's, unchanged: per lattice k_window_tiles leaves tiles[T][U], so a row's candidates are
 * the contiguous slice q in [0, W), W = window * n_users, source tiles[f0*U + q], destination tiles[(f0 + lag)*U + q].  Stage 2 by
 * W alone:
 *   W <= 32768  k_markov_rows<P>, P the power of two >= W from 1024: one 256-thread workgroup per row (persistent over the rows),
 *               the keys p*n + c (0xFFFFFFFF absent) sorted in LDS (mk_sort, the unit's own walk of vet_rank.hpp's bitonic network: the
 *               P / 2 pairs of a stage, four in flight per thread — measured about twice as fast as lds_bitonic_sort,
 *               profiles/markov/markov_timing.json); the thread at a run start finds the run's
 *               end by a galloping / binary search and learns from the neighbouring keys whether the run is its source's only
 *               destination; n_p and m_c are LDS integer histograms; the matrix is written by plain stores into the zeroed output;
 *   W >  32768  k_markov_count: the same sort and run lengths per chunk of 32768 candidates, one global integer atomicAdd per run
 *               into a dense u32 [n][n] matrix per row (the workspace, or d_matrix for lattice 0), rows in passes under a 256 MB
 *               budget (vet_test_markov_chunk_rows); then k_markov_cells, one workgroup per row, walks the matrix in index order.
 * Counts are integers and exact in any order; the FP64 sums are taken per thread over positions tid, tid + 256, ... in ascending
 * order, then wave_sum's butterfly, then the four waves in order.  A value's bits depend on the plan, window, lag and the row's
 * frames only — not on stride, the number of rows, the video's length, the rows per pass, the entry point, or whether the matrix
 * was asked for.  No FP atomics.
 * VET_ERR_INVALID (before anything is allocated or launched): lag < 1, lag > n_frames - 1, window < 1, stride < 1,
 * window > n_frames - lag.  VET_ERR_UNSUPPORTED: a lattice of more than 2048 tiles or bins (the key must stay below 2^22), a
 * matrix output of more than 2^31 - 1 cells per call, window * n_users above 2^31 - 1.
 * Profile ids: stage 1 to k_spatial, k_markov_rows / k_markov_count (with the zeroing of the matrices) to k_transition,
 * k_markov_cells to k_wtab, the mean over the lattices to k_finalize.  Asynchronous on `stream` like vet_transition_entropy. */
int vet_transition_markov(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                          int lag, double *d_stats, int32_t *d_matrix, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_transition_markov_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int lag,
                              double *d_stats, int32_t *d_matrix, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_transition_markov_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                               int n_frames, int window, int stride, int lag, double *h_stats, int32_t *h_matrix,
                               int32_t *h_samples);

/* ---- head-motion statistics: the angular speed of the heads, per window and per viewer -------------------
 * Not in the reference, and independent of the lattices: only the plan's direction table is read.  Every call above describes where
 * attention sits on the tiling; this one reports how fast heads turn.
 * Parameters: lag >= 1, window, stride, per_user.  A video of T frames has P = T - lag pairs; pair f is (frame f, frame f + lag).
 * A (pair, viewer) is a SAMPLE when the viewer has a sample in both frames (the frames in between do not matter).  Its angle a, in
 * radians, is the reference's vector_angle_distance (entropy_utils.py:41-63) of the two samples' Vectors with k_angular_distances'
 * arithmetic: with A and B the rows of the plan's unit table (Vector / |Vector|: sqrt of the sum of squares, three divisions),
 *   c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)),   a = acos(min(max(c, -1), 1))   (ocml acos).
 * One departure from the reference: two samples with the SAME Vector (x, y, z equal as numbers, -0.0 == 0.0, whatever their
 * direction ids: the pixels of a pole row of a grid share one Vector) have a = +0.0 exactly and count as STILL.  The reference's
 * arccos of a dot that rounded to 1 - 2^-53 gives 1.5e-8 rad for a head that did not move.  (`still` counts a == 0: the same-Vector
 * samples and, on direction tables with distinct Vectors closer than about 2^-26 rad, those whose clipped dot is 1.  A sample whose
 * angle is NaN — a zero-length Vector in an explicit table — is not a sample.)
 * Layouts:
 *   per_user = 0  pooled: row r pools the samples of pairs [r*stride, r*stride + window) over all viewers.  R = vet_window_rows(P,
 *                 window, stride), Rows = R; window = P is the whole video.  The row's values in position order: pair-major,
 *                 viewer-minor, W = window * n_users positions (absent ones included).
 *   per_user = 1  row (u, r) holds viewer u's own samples of the same pairs: W = window positions in pair order.  Outputs are
 *                 user-major, Rows = n_users * R, row index u * R + r.
 * Outputs per row, N = its samples:
 *   d_stats     [4][Rows] f64, statistic-major: 0 mean = total / N; 1 sd = sqrt(sum (a - mean)^2 / (N - 1)) (ddof = 1, two passes;
 *               N = 1: NaN as numpy gives; an all-still row: +0.0 exactly); 2 max; 3 total = sum a (the path the head travelled)
 *   d_quantiles [Rows][Q] f64: for fraction q, with x the row's angles ascending, pos = q (N - 1), i = floor(pos):
 *               x[i] + (x[i+1] - x[i]) (pos - i), evaluated as fma(x[i+1] - x[i], pos - i, x[i]); x[N-1] where i >= N - 1 (q = 1
 *               is `max` bit for bit).  x[i] and x[i+1] are EXACT order statistics of the row's own values: not a sketch   (nullable)
 *   d_hist      [Rows][B] i32: bin b counts e_b <= a < e_(b+1) for the B + 1 edges e; values outside [e_0, e_B) are not counted;
 *               e_0 = 0.0 takes the still samples                                                                     (nullable)
 *   d_still     [Rows] i32  samples with a == 0                                                                        (nullable)
 *   d_samples   [Rows] i32  N                                                                                          (nullable)
 *   d_status    [2]   {bad, #rows with N = 0}; the call ADDS, the caller zeroes                                        (nullable)
 * h_fractions [Q] (0 <= Q <= 8, each in [0, 1], strictly increasing) and h_edges [B + 1] (0 <= B <= 64, finite, strictly ascending,
 * radians) are HOST arrays in every entry, consumed before the call returns.  Q = 0 / B = 0 (or a NULL output) skip that output.
 * A row with N = 0 has NaN stats and quantiles, a zero histogram and still = samples = 0: data, not an error.
 * FP sums follow one fixed order that depends on the row only: the row's W positions are cut into blocks of 1024 from its start; in a
 * block, thread t of 256 adds its positions t, t + 256, t + 512, t + 768 in that order (an absent position adds nothing), the 64
 * lanes of a wave combine by wave_sum's butterfly (offsets 32, 16, 8, 4, 2, 1), the four waves are added in order, and the blocks are
 * added in ascending order.  `total` sums a; sd sums fma(d, d, acc) with d = a - mean per position by the same rule.  Counts, the
 * maximum and the histogram are integers or order-free.  A value's bits depend on the plan, lag, window, the layout and the row's
 * frames only — not on stride, the number of rows, the video's length, the entry point, which optional outputs were asked for, the
 * other fractions, or vet_test_motion_lds_values.  No FP atomics.
 * Stage 1, k_motion_angles: one angle per (pair, viewer), NaN = absent, [P][U] (pooled; the samples quantised by sample_dir) or
 * [U][P] (per viewer; behind k_user_dirs' transposed ids), so a row is a contiguous slice of the array in both layouts.  Stage 2 by
 * W alone: W <= 64: k_motion_wave, one wave per row (lane t holds position t; the block rule with one busy wave; the bit patterns
 * sorted across the lanes by a bitonic network of shuffles).  W <= 16384: k_motion_rows, one 256-thread workgroup per row (persistent over the rows): two walks for the sums, the u64
 * bit patterns (non-negative doubles order as their bits) sorted in LDS by lds_bitonic_sort, the quantiles read off.  W > 16384:
 * chunks of 16384 positions, one workgroup each (k_motion_chunk), rows in passes under a 256 MB workspace budget; partial sums per
 * block, combined in order by k_motion_select; the order statistics by a radix selection of the bit patterns, most significant digit
 * first, eight passes of eight bits: a pass counts, for each distinct prefix the wanted ranks still share (at most 16), the next
 * digit of the values under it (integer atomics), and k_motion_select narrows every rank to its digit; after the eighth pass the
 * prefix is the value.  Exact whatever the ties.  Not built: several short rows per wave (a row of 20 values leaves 44 lanes idle); bucket
 * histograms shared between overlapping stride-1 rows (each row is selected on its own).
 * VET_ERR_INVALID (before anything is allocated or launched): lag < 1, lag > n_frames - 1, window < 1, window > n_frames - lag,
 * stride < 1, Q outside [0, 8] or fractions not strictly increasing in [0, 1], B outside [0, 64] or edges not strictly ascending.
 * VET_ERR_UNSUPPORTED: window * n_users above 2^31 - 1; per_user with more than 65535 * 64 frames.
 * Profile ids: stage 1 (with k_user_dirs) to k_spatial, the row kernels to k_transition.  Asynchronous on `stream`. */
int vet_head_motion(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride, int lag,
                    int per_user, const double *h_fractions, int Q, const double *h_edges, int B, double *d_stats,
                    double *d_quantiles, int32_t *d_hist, int32_t *d_still, int32_t *d_samples, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_head_motion_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int lag, int per_user,
                        const double *h_fractions, int Q, const double *h_edges, int B, double *d_stats, double *d_quantiles,
                        int32_t *d_hist, int32_t *d_still, int32_t *d_samples, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_head_motion_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                         int window, int stride, int lag, int per_user, const double *h_fractions, int Q, const double *h_edges, int B,
                         double *h_stats, double *h_quantiles, int32_t *h_hist, int32_t *h_still, int32_t *h_samples);

/* ---- audience dispersion: pairwise viewer angles per window and per viewer --------------------------------
 * Not in the reference, and independent of the lattices: only the plan's direction table is read.  vet_head_motion describes each
 * head on its own; this call reports how tightly the audience looks together in a frame, and which viewers are off on their own.
 * A viewer is PRESENT in frame f exactly as in vet_head_motion (a sample that is not NaN and lies in [0, 1]; a direction id >= 0
 * below the table's size); a sample outside is absent and counted in status[0].  V_f = the viewers present in frame f.
 * A PAIR SAMPLE is (f, {u, v}) with u < v and both present in frame f.  Its angle a(u, v), in radians, is vet_head_motion's angle of
 * the two direction ids: with A and B the rows of the plan's unit table,
 *   c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)),   a = acos(min(max(c, -1), 1))   (ocml acos),
 * and +0.0 exactly when the two Vectors are equal as numbers (SAME; whatever their direction ids).  A NaN angle (a zero-length
 * Vector in an explicit table) is not a sample.  a(u, v) and a(v, u) have the same bits: the products commute and the fused dot
 * adds them in one order; the kernel relies on it.  The PARTNERS of u in f are the v != u of V_f with a(u, v) not NaN.
 * window and stride count frames; R = vet_window_rows(n_frames, window, stride); row r covers frames [r*stride, r*stride + window).
 * Per (frame, viewer) with u in V_f:  s(f, u) = the sum of a(u, v) over u's partners in ASCENDING v (a sequential sum from +0.0),
 * m(f, u) = the smallest, x(f, u) = the largest, k(f, u) = their number, z(f, u) = those with a == 0.
 * Layouts:
 *   per_user = 0  pooled, Rows = R.  Over the row's pair samples, N of them:
 *                 mean = (sum of s(f, u) over the row) / (2 N): every pair sample enters the sum from both sides;
 *                 max = the audience's angular diameter; same = #{a == 0}; hist[b] = #{e_b <= a < e_(b+1)} for the B + 1 host
 *                 edges e in radians (vet_head_motion's d_hist rules: half-open bins, values outside [e_0, e_B) not counted);
 *                 slots = #{(f, u): k(f, u) > 0}; nearest = (sum of m(f, u) over those) / slots, the mean nearest-neighbour
 *                 angle: small for a clustered crowd even when `mean` is large because there are two clusters;
 *                 present = sum_f |V_f|; centroid = the sum of the unit vectors of all present (f, u), lone viewers included (a
 *                 NaN unit vector adds nothing).  |centroid| / present is the resultant length.
 *   per_user = 1  Rows = n_users * R, row index u * R + r: the same from viewer u's side.  samples = sum_f k(f, u);
 *                 mean = sum_f s(f, u) / samples; max = the farthest partner; slots = the frames in which u has a partner;
 *                 nearest = sum_f m(f, u) / slots; same = sum_f z(f, u); present = the frames u is in; centroid = the sum of u's
 *                 own unit vectors (|centroid| / present near 1: a viewer who stays put).  No histogram: per_user with B > 0 is
 *                 VET_ERR_INVALID.  Summed over u, samples = 2 N and same = 2 * same of the pooled row (integers, exact).
 * Outputs, each nullable:
 *   d_stats    [3][Rows] f64, statistic-major: 0 mean, 1 max, 2 nearest
 *   d_centroid [Rows][3] f64
 *   d_hist     [Rows][B] i64
 *   d_counts   [4][Rows] i64: 0 samples (N), 1 same, 2 slots, 3 present (i64: a pooled whole-video row of 1024 viewers x 30000
 *              frames holds 1.57e10 pairs)
 *   d_status   [2] i32 {bad, #rows with N = 0}; the call ADDS, the caller zeroes
 * h_edges [B + 1] (0 <= B <= 64, finite, strictly ascending, radians) is a HOST array in every entry, consumed before the call
 * returns.  B = 0 (or d_hist NULL) skips the histogram.
 * A row with N = 0 (never two viewers in one frame; n_users = 1 is legal) has NaN mean / max / nearest, a zero histogram and
 * samples = same = slots = 0: data, not an error.  Its present and centroid are still filled; a row with present = 0 has a +0.0
 * centroid.
 * FP sums follow one fixed order that depends on the row only.  Inside a frame: s(f, u) as above.  Over the row: vet_head_motion's
 * rule on the row's POSITIONS — pooled: frame-major, viewer-minor, W = window * n_users (absent ones included); per viewer: W =
 * window in frame order.  The positions are cut into blocks of 1024 from the row's start; in a block, thread t of 256 adds its
 * positions t, t + 256, t + 512, t + 768 in that order (an absent position, or for s and m one without a partner, adds nothing),
 * the 64 lanes of a wave combine by wave_sum's butterfly (offsets 32, 16, 8, 4, 2, 1), the four waves are added in order, and the
 * blocks are added in ascending order.  Five sums go by this rule: s, m and the three centroid components.  Counts, the maximum
 * and the histograms are integers or order-free.  A value's bits depend on the plan, window, the layout and the row's frames only —
 * not on stride, the number of rows, the video's length, the entry point, which optional outputs were asked for, the edges, or
 * vet_test_dispersion_tile.  No FP atomics.
 * Stage 1, k_dispersion_pairs: workgroup = (frame, 256 viewers), thread = viewer u; the frame's samples are quantised and their unit
 * vectors staged in LDS in tiles of 1024 viewers (32 B each); the thread walks the partners in ascending v (every lane reads the same
 * LDS address: a broadcast) with s, m, x, k, z in registers and leaves them per (frame, viewer) — [T][U], or [U][T] for the per-viewer
 * layout, so a row is a contiguous slice — with the frame's edge histogram (up to 8 bins: the counts of a >= e_k in registers,
 * differenced; more: a private LDS column per thread; then integer adds).  It walks ALL ORDERED PAIRS, twice the acos, with no
 * cross-lane step; walking the upper triangle and crediting the partner was NOT built and the two were not measured against each
 * other.  Stage 2: k_dispersion_chunk (16 blocks of a row per workgroup: block totals, the row's integers by integer atomics),
 * k_dispersion_finish (one wave per row: the blocks in order, the frames' histograms added and halved); rows in passes under a 256 MB
 * workspace budget.  Overlapping windows never recompute a frame.
 * Workspace: 36 B per (frame, viewer).  Not built: collapsing a frame to (direction, multiplicity) before the walk; the upper
 * triangle; one wave per short row in stage 2 (a per-viewer row of 20 positions takes a workgroup).
 * VET_ERR_INVALID (before anything is allocated or launched): window < 1, window > n_frames, stride < 1, B outside [0, 64], edges
 * not finite and strictly ascending, per_user with B > 0.  VET_ERR_UNSUPPORTED: n_users > 65535 (a frame's pair count must fit 31
 * bits); n_frames * ceil(n_users / 256) above 2^31 - 1.
 * Profile ids: k_dispersion_pairs to k_spatial, stage 2 to k_transition.  Asynchronous on `stream`. */
int vet_dispersion(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                   int per_user, const double *h_edges, int B, double *d_stats, double *d_centroid, int64_t *d_hist,
                   int64_t *d_counts, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_dispersion_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int per_user,
                       const double *h_edges, int B, double *d_stats, double *d_centroid, int64_t *d_hist, int64_t *d_counts,
                       int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_dispersion_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                        int window, int stride, int per_user, const double *h_edges, int B, double *h_stats, double *h_centroid,
                        int64_t *h_hist, int64_t *h_counts);

/* ---- viewer clusters: who looks together, per window -------------------------------------------------------
 * Not in the reference, and independent of the lattices: only the plan's direction table is read.  vet_dispersion says how far apart
 * the viewers are; this call names the groups: which viewers could share one viewport stream in a segment, how many streams the
 * audience needs, and which viewers belong to none.  It is the clustering of viewers by the geodesic distance of their viewport
 * centres of the 360-degree streaming literature; the threshold is the caller's (the Python layer's default of 30 degrees is a
 * choice for head-direction data, not taken from the reference, which has no such call).
 * PRESENCE, samples, direction ids and rows exactly as in vet_dispersion: an absent or out-of-range sample is absent and counted in
 * status[0]; R = vet_window_rows(n_frames, window, stride); row r covers frames [r*stride, r*stride + window).
 * NEAR.  In frame f two present viewers u != v are NEAR if their direction ids are equal, or vet_dispersion's SAME rule applies (the
 * two Vectors are equal as numbers, whatever their ids), or c >= cos_threshold with, A and B the rows of the plan's unit table,
 *   c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)).
 * There is no acos.  A NaN c is not near.  NEAR is symmetric bit for bit: the products commute and the fused dot adds them in one
 * order.  cos_threshold is a double in [-1, 1]: the caller takes the cosine of its angle once (Python: math.cos(math.radians(
 * threshold_deg)), reported in attrs["cos_threshold"]), so no two libms decide one link.
 * LINKED.  For row r and a pair {u, v}: co = the number of the row's frames in which both are present, near = the number of those in
 * which they are NEAR; they are LINKED iff co >= 1 and (double)near >= min_share * (double)co, 0 < min_share <= 1 — one IEEE
 * multiply and one compare.  window = 1: NEAR in that frame.  min_share = 1: within the threshold whenever both are there, the
 * segment rule of the clustering literature.
 * CLUSTERS.  The viewers of a row are those present in at least one of its frames, P of them.  Its clusters are the connected
 * components of the LINKED graph on them; a viewer without a link is a cluster of one (a singleton); a viewer never present has
 * label -1.  Clusters are numbered 0, 1, ... in ascending order of their smallest member's index, K of them: the labels are a
 * function of the row alone.
 * Outputs, each nullable:
 *   d_labels    [R][U] i32
 *   d_sizes     [R][U] i32: the members of cluster k, zero beyond K
 *   d_counts    [5][R] i64, count-major: 0 viewers (P), 1 clusters (K), 2 the largest cluster's size, 3 singletons, 4 links (unordered
 *               LINKED pairs)
 *   d_top       [R][Q] i32: the smallest number of clusters, largest first and equal sizes by label, whose sizes sum to s with
 *               (double)s >= fractions[i] * (double)P — how many viewport streams serve that share of the row's audience (vet_coverage's
 *               `tiles`, over viewers instead of tiles); 0 for P = 0.  0 <= Q <= 16; h_fractions [Q], each in (0, 1], is a HOST array
 *               in every entry, consumed before the call returns.  Q = 0 (or d_top NULL) skips it.
 *   d_stats     [3][R] f64: 0 the partition entropy H = log2 P - (sum_k s_k log2 s_k) / P in bits (ocml log2), the sum by
 *               vet_head_motion's summation rule with the cluster labels k = 0 .. K - 1 as the positions (blocks of 1024 from 0; in a
 *               block thread t of 256 adds positions t, t + 256, t + 512, t + 768, the 64 lanes of a wave combine by wave_sum's
 *               butterfly, the four waves are added in order, the blocks ascending); 1 H / log2 P (NaN for P <= 1); 2 largest / P
 *   d_centroids [R][U][3] f64: for cluster k the sum of the unit vectors of its members' present samples in the row, frame-major then
 *               viewer ascending, a sequential sum from +0.0; entries beyond K are zero; a NaN unit vector adds nothing.  Divide by
 *               the norm for the direction the cluster looks in.
 *   d_links     [R][U][ceil(U / 64)] u64: bit v mod 64 of word v / 64 of row u is LINKED(u, v); the diagonal is zero, the matrix is
 *               symmetric, the bits at and beyond U are zero
 *   d_status    [2] i32 {bad, #rows with P = 0}; the call ADDS, the caller zeroes
 * A row with P = 0 has labels -1, zero counts, sizes and centroids and NaN stats: data, not an error.
 * A value's bits depend on the plan, window, cos_threshold, min_share and the row's frames only — not on stride, the number of rows,
 * the video's length, the entry point, which optional outputs were asked for, the other fractions, or vet_test_cluster_tile.
 * Stage 0, k_cluster_ids: the samples quantised to direction ids [T][U] once.  Stage 1, k_cluster_links: workgroup = (row, 256
 * viewers u, a tile of up to 128 partners v — fewer, a multiple of 8, where a pass has few rows), lane = viewer u, a wave = 64 consecutive u; the partners' records (unit vector and id,
 * 32 B) of a chunk of the row's frames are staged in LDS one per thread (8 partners x 32 frames of a long window; up to 256 / window
 * partners of a window of at most 32 frames), the lane walks the frames with (co, near) of 8 partners in registers (every lane reads
 * the same LDS address: a broadcast), decides LINKED, and one __ballot of the wave is the word links[v][u / 64], stored by one lane.
 * No atomics, no scratch, 8 KB of LDS, no acos.  It walks ALL ORDERED PAIRS; walking the upper triangle and mirroring the words was
 * NOT built and the two were not measured against each other.  Stage 2, k_cluster_components: one 256-thread workgroup per row, the
 * labels in LDS (12 B per viewer, rounded up to a power of two: 96 KB at 8192 viewers): label propagation over the set bits of the
 * link words with pointer jumping until a sweep changes nothing (the fixpoint is each component's smallest member whatever the
 * schedule), the roots ranked by a block prefix sum, sizes by integer LDS atomics, the (size descending, label ascending) records
 * sorted in LDS, the entropy sum by the rule above, and — only when d_centroids is given — a thread per cluster over the row's
 * positions.  Rows run in passes under a 256 MB budget of link words (n_users * ceil(n_users / 64) * 8 B per row; written straight
 * into d_links when that is given).  Workspace besides: 4 B per (frame, viewer).
 * Not built: complete-linkage or clique clusters; a lag band of partition agreement between windows; clusters carried across
 * overlapping windows (every row is clustered on its own, and overlapping windows recompute their shared frames); more than 8192
 * viewers.
 * VET_ERR_INVALID (before anything is allocated or launched): window < 1, window > n_frames, stride < 1, Q outside [0, 16], a
 * fraction outside (0, 1] or NaN, min_share outside (0, 1] or NaN, cos_threshold outside [-1, 1] or NaN.  VET_ERR_UNSUPPORTED:
 * n_users > 8192 (the labels of a row live in LDS); n_frames * ceil(n_users / 256) above 2^31 - 1.
 * Profile ids: k_cluster_ids to k_spatial, k_cluster_links to k_transition, k_cluster_components to k_finalize.  Asynchronous on
 * `stream`. */
int vet_viewer_clusters(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                        double cos_threshold, double min_share, const double *h_fractions, int Q, int32_t *d_labels, int32_t *d_sizes,
                        int64_t *d_counts, int32_t *d_top, double *d_stats, double *d_centroids, uint64_t *d_links, int32_t *d_status,
                        void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_viewer_clusters_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                            double cos_threshold, double min_share, const double *h_fractions, int Q, int32_t *d_labels,
                            int32_t *d_sizes, int64_t *d_counts, int32_t *d_top, double *d_stats, double *d_centroids,
                            uint64_t *d_links, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_viewer_clusters_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                             int window, int stride, double cos_threshold, double min_share, const double *h_fractions, int Q,
                             int32_t *h_labels, int32_t *h_sizes, int64_t *h_counts, int32_t *h_top, double *h_stats,
                             double *h_centroids, uint64_t *h_links);
/* Diagnostic: h_sweeps [2] = the most label-propagation sweeps a row of the plan's context's last vet_viewer_clusters* call took,
 * and their sum over its rows (zeros before any call).  Synchronises the device. */
int vet_viewer_clusters_sweeps(vet_plan *plan, int64_t *h_sweeps);

/* ---- fixation and tile-dwell events: per-viewer runs of a steady viewport ---------------------------------
 * Not in the reference.  The calls above describe where attention sits and how fast heads turn; this one segments each viewer's
 * trajectory in time: when a viewer holds still and for how long (fixations, the velocity-threshold rule I-VT), or how long a viewer
 * stays on one tile (tile dwell).
 * Parameters: mode, cos_threshold, min_frames >= 1, window, stride, per_user.
 * PRESENCE, samples and direction ids exactly as in vet_head_motion.
 * HOLD.  The pair (f, f + 1) of viewer u HOLDS when u is present in both frames and
 *   mode 0 (fixations)  the two directions are NEAR as in vet_viewer_clusters: the same direction id, the same Vector under another
 *                       id, or c = fma(A.z, B.z, fma(A.y, B.y, A.x * B.x)) >= cos_threshold for their rows A, B of the plan's unit
 *                       table.  No acos: cos_threshold = cos of the largest step between two frames, taken once by the caller.
 *   mode 1 (tile dwell) the two samples have the same nearest tile t of lattice 0 (the plan's nearest-tile table, as the per-viewer
 *                       counts read it), t < n_0.  cos_threshold is ignored.
 * RUN.  A run of viewer u is a maximal interval of frames [s, e] in which u is present throughout and every pair inside holds.
 * Every present frame lies in exactly one run; L = e - s + 1.  With n_frames = 1 there is no pair and a present frame is a run of 1.
 * EVENT.  A run with L >= min_frames is an event: a fixation, or a dwell.  Runs are never cut at row boundaries: an event belongs
 * to the row that contains its START frame, with its full length.
 * Layouts:
 *   per_user = 0  pooled: row r takes frames [r*stride, r*stride + window) of all viewers.  R = vet_window_rows(n_frames, window,
 *                 stride), Rows = R; window = n_frames is the whole video.
 *   per_user = 1  row (u, r) holds viewer u's own frames.  Outputs are user-major, Rows = n_users * R, row index u * R + r.
 * Outputs, every one nullable:
 *   d_counts    [5][Rows] i64, statistic-major: 0 samples: the present (viewer, frame) positions of the row; 1 fix_frames: those
 *               positions that lie in an event, wherever the event started; 2 events: the events that start in the row; 3 sum_len:
 *               the sum of their L; 4 max_len: the largest L, 0 when there is none
 *   d_hist      [Rows][B] i32: bin b counts the row's events with e_b <= L < e_(b+1).  h_edges [B + 1] is a HOST i32 array in
 *               every entry, consumed before the call returns: 0 <= B <= 64, edges >= 1 and strictly ascending.  B = 0 skips it
 *   d_labels    [n_users][n_frames] i32: L of the event the sample lies in; 0 where the sample is present but its run is shorter
 *               than min_frames; -1 where it is absent.  Independent of window, stride and the layout
 *   d_offsets   [n_users + 1] i64: the exclusive prefix of the viewers' event counts over the whole video; offsets[n_users] is
 *               the number of events
 *   d_events    [max_events][4] i32: (viewer, start, L, the direction id of the sample at frame start + (L - 1) / 2), ordered by
 *               viewer, then start.  Only the first max_events events are written; d_offsets[n_users] always says how many there are
 *   d_centroids [max_events][3] f64, needs d_events: per listed event the sum of the unit vectors of its frames in ascending frame
 *               order, one accumulator per component from +0.0, plain adds
 *   d_status    [2]   {bad, #rows without a sample}; the call ADDS, the caller zeroes
 * A row without a sample has zero counts and a zero histogram: data, not an error.  No NaN exists in this call.
 * Everything is an integer except the centroids, and a centroid's bits depend on the plan and the event's own frames only.  No
 * output depends on stride, the number of rows, the layout, the entry point, which optional outputs were asked for, the order of
 * the viewer columns, or vet_test_fixation_chunk: under a permutation of the viewer columns the pooled rows are equal and the
 * per-viewer rows, labels and events permute.  Integer atomics only; no FP atomics.
 * Stage 1, k_user_dirs: the direction ids transposed to [U][T], for both layouts.  k_fix_runs: one 256-thread workgroup per viewer,
 * persistent over the viewers, walks the viewer's frames in chunks of 1024, four consecutive frames per thread; the start of a
 * frame's run is an inclusive max-scan of "f where a run starts at f" — inside the thread, across the lanes by shuffles, across the
 * four waves through LDS words, the carry into the next chunk in a register, so a run may span any number of chunks; the thread
 * that holds a run's END writes L at the run's start (4 B per sample of workspace).  k_fix_offsets: the exclusive prefix of the
 * viewers' event counts.  k_fix_labels: the same walk, scan and carry give every sample its label, and a sum-scan of the qualifying
 * starts an event's rank inside its viewer, hence its slot in the list.  k_fix_centroids: one thread per listed event.  Rows:
 * per viewer a wave (windows of up to 512 frames) or a workgroup per row sums the row's labels and lengths, the histogram in LDS;
 * pooled, k_fix_frames (workgroup = 256 frames x 64 viewers, lane = frame) adds each frame's totals by integer atomics, the histogram
 * by one integer atomic per (event, row that holds its start), and the same row kernel sums a row's frames.  Workspace: 12 B per
 * sample (8 B with d_labels), 24 B per frame of the pooled layout.
 * Not built: dispersion-threshold (I-DT) fixations; a velocity estimate over a lag of more than one frame; saccade amplitudes
 * between consecutive events; merging events across short absences; dwell on lattices other than the first; quantiles of the
 * durations (the histogram is exact; quantiles would need a sort per row); a decoupled look-back scan for audiences of fewer viewers
 * than the device has CUs (one workgroup walks one viewer); several short rows per wave; a per-workgroup LDS histogram in front of
 * the pooled layout's histogram atomics (the whole video as one pooled row is the slow shape: README.md).
 * VET_ERR_INVALID (before anything is allocated or launched): window < 1, window > n_frames, stride < 1, min_frames < 1, mode not 0
 * or 1, cos_threshold NaN, B outside [0, 64], an edge below 1 or edges not strictly ascending, max_events < 0, d_centroids without
 * d_events.  VET_ERR_UNSUPPORTED: window * n_users above 2^31 - 1; more than 65535 * 64 frames; mode 1 on a plan whose lattice 0
 * the per-viewer count path does not take (4 n_0 bytes beyond the LDS).
 * Profile ids: k_user_dirs to k_spatial, the walks, the prefix and the centroids to k_transition, the frame totals and the rows to
 * k_finalize.  Asynchronous on `stream`. */
int vet_fixations(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride, int mode,
                  double cos_threshold, int min_frames, int per_user, const int32_t *h_edges, int B, int64_t max_events,
                  int64_t *d_counts, int32_t *d_hist, int32_t *d_labels, int64_t *d_offsets, int32_t *d_events, double *d_centroids,
                  int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_fixations_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int mode,
                      double cos_threshold, int min_frames, int per_user, const int32_t *h_edges, int B, int64_t max_events,
                      int64_t *d_counts, int32_t *d_hist, int32_t *d_labels, int64_t *d_offsets, int32_t *d_events,
                      double *d_centroids, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa.  The event outputs take a second call: a first call
 * with max_events = 0 and h_offsets gives their number. */
int vet_fixations_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                       int window, int stride, int mode, double cos_threshold, int min_frames, int per_user, const int32_t *h_edges,
                       int B, int64_t max_events, int64_t *h_counts, int32_t *h_hist, int32_t *h_labels, int64_t *h_offsets,
                       int32_t *h_events, double *h_centroids);

/* ---- saliency maps: the spherical kernel density of attention per window and per viewer ------------------
 * Not in the reference, and independent of the lattices: only the plan's direction table is read.  The continuous counterpart of
 * the tile heatmaps: a smooth density of viewing directions on the sphere per segment of the video, comparable across tilings.
 * PRESENCE, samples and direction ids exactly as in vet_head_motion / vet_dispersion: an absent sample, or one outside [0, 1] (an id
 * at or beyond the table's size), is counted in status[0] and contributes nothing.
 * MAP GRID: W x H cells, equirectangular, laid out as vet_heatmap_create lays out pixels: column c has lon = (c + 0.5) / W * 360 -
 * 180, row y has lat = 90 - (y + 0.5) / H * 180 (row 0 is the top).  P(c, y) is the unrounded Vector.from_spherical(lon, lat) of the
 * cell centre by the heatmap's arithmetic: theta = lon * (pi / 180), phi = (90 - lat) * (pi / 180), x = sin(phi) cos(theta),
 * y = sin(phi) sin(theta), z = cos(phi), divided by sqrt(x*x + y*y + z*z) (no fused operation).  The W cosines and sines of theta and
 * the H sines and cosines of phi are taken ONCE ON THE HOST (the C library's sin / cos) and the products, the root and the
 * divisions on the device.  The cell's share of the sphere is a_y = (cos(pi*y/H) - cos(pi*(y+1)/H)) / (2*W), a host-built [H] FP64
 * table (sum over the map: 1).
 * KERNEL: kappa = 1 / sigma^2, sigma in radians, computed once on the host in FP64.  With A a row of the plan's unit table (as in
 * vet_head_motion):  c = fma(P.z, A.z, fma(P.y, A.y, P.x * A.x)),  k(P, A) = exp(kappa * (c - 1))  (ocml exp; the product and the
 * difference are not fused) — the von Mises-Fisher kernel, for small angles the Gaussian exp(-theta^2 / (2 sigma^2)).  Smooth over
 * the whole sphere, no acos, NO TRUNCATION: a cut-off radius would make the value discontinuous in c.
 * ROWS: R = vet_window_rows(n_frames, window, stride); row r covers frames [r*stride, r*stride + window).  per_user = 0: the row
 * pools all viewers, Rows = R.  per_user = 1: Rows = n_users * R, row index u * R + r, viewer u's own samples.  The row's LIST is the
 * distinct direction ids among its present samples in ASCENDING id, each with its multiplicity m (an integer).  Ids are collapsed by
 * id, not by Vector equality: pole ids that share a Vector stay separate entries.  N = sum of m; distinct = the list's length.
 * MAP VALUE: S(r, p) starts at +0.0; over the LIST in ascending id, S = fma((double)m, k(P_p, A_id), S) — one sequential sum per
 * pixel.  M(r, p) = S * g_r: scale 0: g = 1 and the multiply is skipped; scale 1: g = 1 / (double)N; scale 2: g = C / (double)N with
 * C = kappa / (2 pi (1 - exp(-2 kappa))), a host FP64 constant: a density per steradian whose integral is 1.  g is one division, the
 * product one multiply.
 * ROW STATISTICS, from M.  FP sums use vet_head_motion's rule with the map's pixels in row-major order as the positions: blocks of
 * 1024, thread t of 256 adds t, t + 256, t + 512, t + 768 in that order, the lanes combine by wave_sum, then the four waves in
 * order, then the blocks in ascending order.
 *   mass       = sum_p M_p * a_y, the map's mean over the sphere (a_y is a share: the a_y of all cells add up to 1).  At scale 2,
 *              a density per steradian, 4 pi * mass is the integral over the sphere: close to 1, mass close to 1 / (4 pi) =
 *              0.0796, when the grid resolves sigma — the caller's resolution check
 *   peak       = the largest M_p; peak_index = the smallest pixel index (y * W + c) that holds it
 *   entropy    with w_p = M_p * a_y and Wsum = sum_p w_p (the rule; the same bits as mass): q_p = w_p / Wsum,
 *              t_p = q_p * log2(q_p / a_y) (ocml log2), 0 where w_p == 0; entropy = -(sum_p t_p) by the rule.  Bits; <= 0 up to
 *              rounding; 0 = uniform over the sphere
 *   area       = exp2(entropy), the effective share of the sphere (per viewer: the exploration ratio)
 * A row with N = 0 has a +0.0 map, NaN statistics, peak_index = -1, samples = distinct = 0: data, not an error; counted in status[1].
 * A value's bits depend on the plan, W, H, sigma, scale, window, the layout and the row's frames only — not on stride, the number of
 * rows, the video's length, the entry point, which optional outputs were asked for, the row chunk, or vet_test_saliency_tile.  No FP
 * atomics.
 * Outputs, each nullable:
 *   d_map      [Rows][H][W] f64: M
 *   d_stats    [4][Rows] f64, statistic-major: 0 mass, 1 peak, 2 entropy, 3 area
 *   d_peak     [Rows] i32: peak_index
 *   d_counts   [2][Rows] i64: 0 samples (N), 1 distinct
 *   d_status   [2] i32 {bad, #rows with N = 0}; the call ADDS, the caller zeroes
 * With d_map NULL nothing of [Rows][H][W] exists: the maps of a pass of rows live in the workspace, and a pass (its lists, and its
 * maps when d_map is NULL) stays under a 256 MB budget.  With d_map, d_stats and d_peak all NULL no map is computed.
 * Stages: the samples quantised once into direction ids ([T][U]; per viewer k_user_dirs' transposed [U][T], so a row is a contiguous
 * slice in both); the lists — rows of up to 4096 positions by k_saliency_sort (one workgroup per row: LDS bitonic sort, run lengths),
 * longer rows by integer atomics into a dense u32 [D] row (tables of up to 32768 directions: per workgroup in LDS first) and
 * k_saliency_compact in ascending id; k_saliency_map — workgroup = (row,
 * 256 pixels), thread = pixel with P in registers, the list staged in LDS in tiles of 1024 entries (32 B: unit vector and the
 * multiplicity as a double; every lane reads the same address, a broadcast), S in a register across tiles: 69 VGPRs, no scratch,
 * 32 KB LDS, 5 waves per SIMD (LDS-bound); k_saliency_rows — one workgroup per row.  Overlapping windows rebuild each row's list.
 * Workspace: 4 B per sample + per row of a pass 8 B per list slot (min(positions, directions)), the dense counts on the long path.
 * VET_ERR_INVALID (before anything is allocated or launched): window < 1, window > n_frames, stride < 1, sigma_rad not finite, <= 0
 * or > pi, W outside [2, 4096], H outside [1, 2048], scale outside {0, 1, 2}.  VET_ERR_UNSUPPORTED: pooled, n_frames * n_users above
 * 256 * (2^31 - 1) (one workgroup per 256 samples); per viewer, n_frames above 65535 * 64 (k_user_dirs' grid).
 * Profile ids: k_saliency_map to k_spatial, the other stages to k_transition.  Asynchronous on `stream`. */
int vet_saliency(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                 int per_user, double sigma_rad, int W, int H, int scale, double *d_map, double *d_stats, int32_t *d_peak,
                 int64_t *d_counts, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_saliency_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, int per_user,
                     double sigma_rad, int W, int H, int scale, double *d_map, double *d_stats, int32_t *d_peak, int64_t *d_counts,
                     int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_saliency_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                      int window, int stride, int per_user, double sigma_rad, int W, int H, int scale, double *h_map, double *h_stats,
                      int32_t *h_peak, int64_t *h_counts);

/* ---- saliency similarity: CC, SIM, JSD, KL and NSS between the saliency maps of two audiences ------------------
 * Not in the reference.  The two-audience question of vet_group_divergence asked of the tiling-free maps of vet_saliency: per
 * window of frames, how alike are the densities of where audience A and audience B look.
 * ROWS, PRESENCE, ids, MAP GRID, the KERNEL k(P, A), kappa, C and the summation RULE exactly as vet_saliency, pooled layout (the rule:
 * blocks of 1024 positions, thread t of 256 adds t, t + 256, t + 512, t + 768, then wave_sum, the four waves in order, the blocks
 * ascending).  There is no per_user and no scale: the maps are scale 2 (density); every value below is scale-free in exact arithmetic.
 * AUDIENCES: groups is a HOST array [n_users] in every entry, read before the call returns: 0 = audience A, 1 = audience B, any
 * other value = excluded.  Audience g of row r is the row's present samples of the viewers labelled g; its list, N_g, distinct_g and
 * map M^g are vet_saliency's — the maps are bit for bit what vet_saliency_ids returns at scale 2 on ids in which every other viewer's
 * samples are -1 — and mass_g is its mass (the same rule, the same bits).  status[0] counts the out-of-range samples of ALL viewers,
 * the excluded ones too (stage 0 runs before the mask); status[1] counts the rows in which an audience is empty.
 * PIXEL SUMS, each by the rule over the pixels in row-major order; a = M^A_p, b = M^B_p, ay the cell's share:
 *   qa = (a*ay)/mass_a, qb = (b*ay)/mass_b;  da = a - mass_a, db = b - mass_b (the mass is the area-weighted mean: the shares add to 1)
 *   va = sum ay*(da*da), vb = sum ay*(db*db), cov = sum ay*(da*db);  cc = cov / sqrt(va*vb)      Pearson's correlation
 *   sim    = sum fmin(qa, qb)                                                                     histogram intersection, in [0, 1]
 *   jsd    = 0.5 * sum (ta + tb), m = 0.5*(qa+qb), ta = qa != 0 ? qa*log2(qa/m) : 0, tb alike     bits, in [0, 1]
 *   kl_ab  = sum (qa != 0 ? qa*log2(qa/qb) : 0); kl_ba the same expression with the roles exchanged (its own log2)
 * Where A has weight on a cell whose B value underflowed to 0.0 the IEEE value of the expression is +inf and so is kl_ab: data, not
 * an error (sigma below about 3 degrees, where 2 kappa exceeds 708).  The products are parenthesised as written: exchanging the two
 * labels exchanges kl_ab <-> kl_ba, nss_ab <-> nss_ba, mass_a <-> mass_b and leaves cc, sim and jsd unchanged, byte for byte.
 * NSS BY POINT EVALUATION (X evaluated on Y's density; nss_ab: X = A, Y = B) — the map is a kernel density, so it is evaluated AT a
 * sample's direction; no sample is assigned to a pixel.  For entry i of X's list (ascending id, unit row A_i, multiplicity m_i):
 * S_i starts at +0.0 and runs over Y's list in ascending id, S_i = fma((double)m_j, k(A_i, B_j), S_i) — the map's inner loop with the
 * cell direction replaced by A_i;  v_i = (double)m_i * (S_i * g_Y), g_Y = C / (double)N_Y;  V = sum_i v_i by the rule over the list
 * positions;  nss_xy = (V / (double)N_X - mass_Y) / sqrt(v_Y), v_Y being Y's va or vb.  Positive: X looks where Y's density is above
 * its sphere average.
 * A row with N_A = 0 or N_B = 0: the seven comparison values are NaN, mass_g is NaN for the empty audience and vet_saliency's value
 * for the other, the counts are as they are.
 * A value's bits depend on the plan, W, H, sigma, window and the row's frames and labels only — not on stride, the number of rows, the
 * video's length, the entry point, which outputs were asked for, the pass a row falls into, vet_test_saliency_tile, the excluded
 * viewers' samples or the order of the viewer columns (lists are in ascending id).  No FP atomics.
 * Outputs, each nullable:
 *   d_maps     [2][Rows][H][W] f64: M^A, then M^B
 *   d_stats    [9][Rows] f64, statistic-major: cc, sim, jsd, kl_ab, kl_ba, nss_ab, nss_ba, mass_a, mass_b
 *   d_counts   [4][Rows] i64: samples_a, samples_b, distinct_a, distinct_b
 *   d_status   [2] i32 {bad, #rows with an empty audience}; the call ADDS, the caller zeroes
 * With d_maps NULL nothing of [Rows][H][W] exists outside a pass: the maps of a pass of rows live in the workspace, and a pass (two
 * lists, two maps when d_maps is NULL, the v_i of both directions per row) stays under the 256 MB budget.  With d_maps and d_stats
 * both NULL no map is computed.
 * Stages: the samples quantised once (k_saliency_ids); k_saliency_mask — one streaming pass writes the two masked [T][U] id arrays
 * (8 B more workspace per sample; the list and map kernels of vet_saliency then run unchanged, for A and for B, per pass);
 * k_saliency_points — workgroup = (row, 256 entries of X's list, direction), thread = entry with its unit vector in registers, Y's
 * list staged in LDS in tiles as k_saliency_map stages it (a broadcast), v_i to the workspace: 77 VGPRs, no scratch, 32 KB LDS,
 * 5 waves per SIMD (LDS-bound); k_saliency_compare — one workgroup per row: the two masses, one pass over both maps with the seven
 * sums carried together (four log2 per pixel, LDS for the wave partials only), the v_i by the rule, the values, the counts and
 * status[1]: 97 VGPRs, no scratch, 224 B LDS, 4 waves per SIMD; k_saliency_mask 14 VGPRs, no scratch.
 * VET_ERR_INVALID (before anything is allocated or launched): everything vet_saliency refuses for the pooled layout, groups NULL, an
 * audience without a viewer.  VET_ERR_UNSUPPORTED as vet_saliency, pooled.
 * Profile ids: k_saliency_map and k_saliency_points to k_spatial, the other stages to k_transition.  Asynchronous on `stream`. */
int vet_saliency_similarity(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                            const int8_t *groups, double sigma_rad, int W, int H, double *d_maps, double *d_stats, int64_t *d_counts,
                            int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_saliency_similarity_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride,
                                const int8_t *groups, double sigma_rad, int W, int H, double *d_maps, double *d_stats,
                                int64_t *d_counts, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_saliency_similarity_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users,
                                 int n_frames, int window, int stride, const int8_t *groups, double sigma_rad, int W, int H,
                                 double *h_maps, double *h_stats, int64_t *h_counts);

/* ---- saliency scoring: AUC, NSS, IG, CC, SIM, KL of a predicted map against where the audience looked ------------------
 * Not in the reference.  The question a saliency toolkit is asked most: here is a map from elsewhere — a model's prediction, another
 * dataset's ground truth, a centre or equator bias, last segment's map — how well does it predict where THIS audience looked, per
 * window of frames.  Pooled layout only.
 * ROWS, PRESENCE, ids, MAP GRID, a_y, the KERNEL k(P, A), kappa, C, the LIST of a row (distinct ids d_i ascending, multiplicities m_i,
 * N = sum m_i) and the summation RULE exactly as vet_saliency, pooled layout (the rule: blocks of 1024 positions, thread t of 256 adds
 * t, t + 256, t + 512, t + 768 to +0.0 in that order, then wave_sum, the four waves in order, the blocks ascending).
 * PREDICTED MAP: pred is [n_pred][H][W] f64, laid out exactly as vet_saliency's maps (row 0 at the top, column c centred at lon
 * (c + 0.5) / W * 360 - 180); n_pred = 1: one static map scores every row; n_pred = R: row r is scored by map r.  PRECONDITION of the
 * device entries: every value finite and non-negative, in any scale (-0.0 is taken as +0.0); the entries read it in place and do not
 * check it.  P is the row's map, P_p a cell, a_p = a_y its share of the sphere.
 * SAMPLING: v_i is P at direction d_i by BILINEAR interpolation on the cell-centre grid.  With (x, y, z) the unit row of the plan's
 * table (as in vet_head_motion) and pi = 3.141592653589793:
 *   lon = (x == 0 && y == 0) ? 0 : atan2(y, x);  fx = (lon + pi) / (2 * pi) * W - 0.5;  c0 = floor(fx), tx = fx - c0;
 *   c0 and c1 = c0 + 1 wrap modulo W;
 *   fy = clamp(acos(clamp(z, -1, 1)) / pi * H - 0.5, 0, H - 1);  y0 = floor(fy), y1 = min(y0 + 1, H - 1), ty = fy - y0;
 *   top = P[y0][c0] + tx * (P[y0][c1] - P[y0][c0]), bot likewise on y1;  v = top + ty * (bot - top)
 * (ocml atan2 and acos; no fused operation).  The a + t * (b - a) form is required: four equal corners return exactly their value, so
 * the AUC's ties on constant regions of a map (zeros above all) are exact.  Interpolation, not "the pixel the sample falls in": on
 * a 100 x 200 sample grid and a 180 x 90 map every tenth longitude lies exactly on a cell border, where a floor is decided by the
 * last bit of atan2; the interpolated value is continuous there.
 * LOCATION METRICS (no audience map is built for them):
 *   mass_pred = sum_p a_p * P_p by the rule over the pixels in row-major order (vet_saliency's mass terms)
 *   var_pred  = sum_p a_p * ((P_p - mass_pred) * (P_p - mass_pred)) by the rule
 *   nss       = (sum_i (double)m_i * v_i / (double)N - mass_pred) / sqrt(var_pred)
 *   info_gain = sum_i (double)m_i * log2(v_i / mass_pred) / (double)N      bits over the uniform sphere (ocml log2); -inf where the map
 *               is 0.0 at a sample: data, not an error
 *   auc       = sum_i (double)m_i * u_i / (double)N,  u_i = L(v_i) + 0.5 * E(v_i),
 *               L(v) = sum_y a_y * #{x : P[y][x] < v},  E(v) = sum_y a_y * #{x : P[y][x] == v}
 * The y sums of L and E run in ascending y as acc = acc + a_y * (double)count from +0.0 (integer counts); the three sums over i run
 * by the rule over the list positions.  STATED DEPARTURE: this AUC is the Mann-Whitney form of AUC-Judd with the WHOLE SPHERE as
 * the negatives and every cell weighted by its area — the probability that a sample's value exceeds that of a uniformly drawn point
 * of the sphere, ties counting a half.  It is not the thresholded trapezoid over unfixated pixels, and it is 0.5 for a constant map.
 * DISTRIBUTION METRICS (want_dist != 0): the audience's density map M is vet_saliency's at scale 2, bit for bit (k_saliency_map,
 * unchanged), mass its mass.  cc, sim, jsd and kl are vet_saliency_similarity's PIXEL SUMS with a = M_p, b = P_p, mass_a = mass,
 * mass_b = mass_pred: cc = cov / sqrt(va*vb), sim = sum fmin(qa, qb), jsd = 0.5 * sum (ta + tb), kl = kl_ab = sum (qa != 0 ?
 * qa*log2(qa/qb) : 0) — the audience from the prediction; +inf where the audience has weight on a cell with P = 0.0.
 * NaN RULES: a row with N = 0 has NaN in the first eight statistics and mass_pred is still the map's; it is counted in status[1].
 * With want_dist = 0, cc, sim, jsd, kl and mass are NaN and no density is evaluated (sigma_rad is still validated).  Beyond that
 * nothing is special-cased: an all-zero or a constant map gives what IEEE gives for the expressions above.
 * A value's bits depend on the plan, the row's predicted map, sigma, window and the row's frames only — not on stride, the number of
 * rows, the video's length, the entry point, which outputs were asked for, want_dist (the location metrics), n_pred (a static map
 * against R copies of it), the pass a row falls into, vet_test_saliency_tile or the order of the viewer columns.  No FP atomics.
 * Outputs, each nullable:
 *   d_map      [R][H][W] f64: M, the audience's map (built whenever d_map is given, also with want_dist = 0)
 *   d_stats    [9][R] f64, statistic-major: auc, nss, info_gain, cc, sim, jsd, kl, mass, mass_pred
 *   d_counts   [2][R] i64: 0 samples (N), 1 distinct
 *   d_status   [2] i32 {bad, #rows with N = 0}; the call ADDS, the caller zeroes
 * Stages: the samples quantised once (k_saliency_ids) and the lists by vet_saliency's list kernels; k_score_sort — workgroup = (map
 * row, map): the row's W bit patterns sorted in LDS by lds_bitonic_sort (non-negative doubles order as their bits, so W <= 4096,
 * 32 KB of keys, needs no second path), a sorted copy [H][W] in the workspace; a static map is sorted once per call;
 * k_score_points — workgroup = (row, 256 list entries), thread = entry: v_i by four loads, then the sorted map rows staged in LDS in
 * tiles of whole map rows (at most 32 KB) and one lower- and one upper-bound binary search per map row, L and E in registers
 * (about H * 2 * log2 W LDS reads per entry instead of W * H compares): 28 VGPRs, no scratch, 32 KB LDS, 5 waves per SIMD
 * (LDS-bound); k_score_rows — one workgroup per row: mass_pred, var_pred, the list sums, with want_dist the audience's mass and the
 * five pixel sums carried together, the values, the counts and status[1]: 93 VGPRs, no scratch, 160 B LDS, 5 waves per SIMD;
 * k_score_sort 10 VGPRs, no scratch, 32 KB LDS, 5 waves per SIMD (LDS-bound).  k_saliency_map runs only with want_dist (and d_stats) or d_map.
 * Workspace: 4 B per sample, the sorted copy of a static map, + per row of a pass 8 B per list slot, 16 B per list slot for v_i and
 * u_i, W*H*8 B for the sorted copy when n_pred = R and for M when d_map is NULL; a pass stays under vet_saliency's 256 MB budget.
 * VET_ERR_INVALID (before anything is allocated or launched): everything vet_saliency refuses for the pooled layout, pred NULL,
 * n_pred other than 1 or R.  VET_ERR_UNSUPPORTED as vet_saliency, pooled.
 * Profile ids: k_saliency_map and k_score_points to k_spatial, the other stages to k_transition.  Asynchronous on `stream`. */
int vet_saliency_score(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                       double sigma_rad, int W, int H, const double *d_pred, int n_pred, int want_dist, double *d_map,
                       double *d_stats, int64_t *d_counts, int32_t *d_status, void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_saliency_score_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, double sigma_rad,
                           int W, int H, const double *d_pred, int n_pred, int want_dist, double *d_map, double *d_stats,
                           int64_t *d_counts, int32_t *d_status, void *stream);
/* Host buffers: H2D (h_pred [n_pred][H][W] is HOST memory here, uploaded with the samples), run, D2H, synchronous; VET_ERR_RANGE when
 * a sample is outside [0, 1] (outputs are still written); never VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice
 * versa. */
int vet_saliency_score_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                            int window, int stride, double sigma_rad, int W, int H, const double *h_pred, int n_pred, int want_dist,
                            double *h_map, double *h_stats, int64_t *h_counts);

/* ---- viewer congruency: the leave-one-out saliency score of every viewer per window ------------------
 * Not in the reference.  Inter-observer congruency: how well the REST of the audience predicts where viewer u looks, per window of
 * frames — the noise ceiling of a saliency model, the outlier detector for viewers, the lattice-free counterpart of
 * vet_crowd_divergence.  No map is built: the others' kernel density is evaluated AT the viewer's own directions, and the mean and
 * variance of that density over the sphere are closed forms of the vMF kernel.
 * ROWS, PRESENCE, ids, the KERNEL k(P, A) = exp(kappa * (c - 1)) with its fused dot c, kappa = 1 / sigma^2, C = kappa / (2 pi (1 -
 * exp(-2 kappa))) and the summation RULE exactly as vet_saliency (the rule: blocks of 1024 positions, thread t of 256 adds t, t + 256,
 * t + 512, t + 768 to +0.0 in that order, then wave_sum, the four waves in order, the blocks ascending).  R = vet_window_rows(n_frames,
 * window, stride); row r covers frames [r*stride, r*stride + window).
 * LISTS of row r: the POOLED list is vet_saliency's (per_user = 0): the distinct ids d_j in ascending id with multiplicities m_j,
 * N = sum m_j.  Viewer u's OWN list is vet_saliency's per-viewer list of the same row: multiplicities a_j, n_u = sum a_j, distinct_u
 * entries.  The OTHERS: N' = N - n_u, w_j = m_j - a_j (a_j = 0 where u does not hold d_j), an integer >= 0, taken as integers.
 * DENSITY OF THE OTHERS at own entry i (unit row A_i): S_i starts at +0.0 and runs over the POOLED list in ascending id,
 * S_i = fma((double)w_j, k(A_i, A_j), S_i); f_i = S_i * g with g = C / (double)N'.  An entry with w_j = 0 adds exactly nothing, so S_i
 * has the bits k_saliency_points produces on the list of everyone but u; no difference of two densities is taken anywhere.
 * OVERLAP of two kernels, G(c) = the integral over the sphere of k(., A_i) k(., A_j):  r = sqrt(fmax(0, fma(2, c, 2))), x = kappa * r;
 * x < 1e-4 (antipodal directions): G = g0 * (1 + (x*x) / 6) with the host constant g0 = 4 pi exp(-2 kappa); otherwise
 * G = ((2 pi * exp(kappa * (r - 2))) * (-expm1(-2 * x))) / x  (ocml sqrt, exp, expm1).  With want_nss the same walk carries, per own
 * entry i,  T_i = fma((double)m_j, G_ij, T_i) over the whole pooled list  and  O_i = fma((double)a_j, G_ij, O_i) over the entries the
 * viewer holds, both from +0.0 in ascending id.  T_i depends on the direction alone: every viewer that holds it has the same bits.
 * PER (u, r), sums over the own entries by the rule with the own-list positions as the positions:
 *   F = sum (double)a_i * f_i;  L = sum (double)a_i * log2(4 pi * f_i)  (ocml log2; 4 pi = 4 * 3.141592653589793);
 *   B_u = sum (double)a_i * T_i;  A_u = sum (double)a_i * O_i
 *   lift      = (4 pi * F) / (double)n_u       the others' density at the viewer's samples relative to the uniform sphere (1 = chance)
 *   info_gain = L / (double)n_u                bits over the uniform baseline; -inf where an S_i underflowed to 0.0: data, not an error
 *   nss       = (F / (double)n_u - mu) / sqrt(v),  mu = 1 / (4 pi),  v = ((g*g) * Q_u) / (4 pi) - mu*mu,  Q_u = (Q - 2 * B_u) + A_u
 *               with Q = sum_j (double)m_j * T_j by the rule over the POOLED list's positions (Q = sum_ij m_i m_j G_ij, so Q_u =
 *               sum_ij w_i w_j G_ij is of Q's size and the subtraction is benign).  v <= 0 or not finite: NaN.
 * A viewer without a sample in the row (n_u = 0) or alone in it (N' = 0) is NOT SCORED: NaN statistics, the counts as they are — data,
 * not an error.
 * PER ROW, by the rule with the viewer index as the position (a viewer that is not scored adds nothing): scored = the scored viewers,
 * and the means lift, info_gain and nss = sum / scored with IEEE propagation (-inf and NaN carry; scored = 0 gives NaN) — the segment's
 * inter-observer congruency.
 * A value's bits depend on the plan, sigma, window and the row's frames only — not on stride, the number of rows, the video's length,
 * the pass a row falls into, vet_test_saliency_tile, the entry point or the outputs asked for; a viewer's own values do not depend on
 * the order of the other viewers' columns (every sum behind them runs over a list in ascending id), the row means do (the rule over
 * the viewer index).  With want_nss = 0 the nss outputs (stats 2, rows 3) are NaN and every other output keeps its bytes.  No FP atomics.
 * Outputs, each nullable (a NULL output is not written):
 *   d_stats    [3][n_users][R] f64, statistic-major, then user-major: 0 lift, 1 info_gain, 2 nss
 *   d_counts   [3][n_users][R] i64: 0 samples (n_u), 1 distinct (distinct_u), 2 others (N')
 *   d_rows     [4][R] f64: 0 scored, 1 mean lift, 2 mean info_gain, 3 mean nss
 *   d_status   [2] i32 {bad, #rows without a scored viewer}; the call ADDS, the caller zeroes
 * Stages: the samples quantised once per layout (k_saliency_ids [T][U], k_user_dirs [U][T]); per pass of rows the pooled lists and
 * every viewer's own lists by vet_saliency's list kernels; k_congruency_points — workgroup = (row, 256 queries), a query = (viewer,
 * one entry of the viewer's own list) on a dense [U][min(window, directions)] grid (a workgroup without an active query returns, a
 * wave without one skips the walk), the pooled list staged in LDS in tiles of 1024 entries of 32 B (unit vector, id, multiplicity;
 * a broadcast), the leave-one-out weight one integer compare per step against the viewer's next own id: 64 VGPRs (96 with want_nss),
 * no scratch, 32 KB LDS, 5 waves per SIMD (LDS-bound); k_congruency_users — one wave per (row, viewer) playing the rule's four waves
 * in turn; k_congruency_rows — one workgroup per row.  With d_stats and d_rows both NULL no density is evaluated.
 * Workspace: 8 B per sample + per row of a pass 8 B per list slot (pooled: min(window * n_users, directions); per viewer: n_users *
 * min(window, directions)), 8 B (24 B with want_nss) per query slot, the dense counts on the long-row path (up to half the budget);
 * a pass stays under vet_saliency's 256 MB budget.
 * VET_ERR_INVALID (before anything is allocated or launched): window < 1, window > n_frames, stride < 1, sigma_rad not finite, <= 0
 * or > pi, n_users < 2.  VET_ERR_UNSUPPORTED as vet_saliency for both layouts.
 * Profile ids: k_congruency_points to k_spatial, the other stages to k_transition.  Asynchronous on `stream`. */
int vet_congruency(vet_plan *plan, const double *d_mu, const double *d_mv, int n_users, int n_frames, int window, int stride,
                   double sigma_rad, int want_nss, double *d_stats, int64_t *d_counts, double *d_rows, int32_t *d_status,
                   void *stream);
/* Same, samples given as direction ids into the plan's direction table (-1 absent). */
int vet_congruency_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames, int window, int stride, double sigma_rad,
                       int want_nss, double *d_stats, int64_t *d_counts, double *d_rows, int32_t *d_status, void *stream);
/* Host buffers: H2D, run, D2H, synchronous; VET_ERR_RANGE when a sample is outside [0, 1] (outputs are still written); never
 * VET_ERR_EMPTY.  h_mu / h_mv may be NULL when h_ids is given and vice versa. */
int vet_congruency_host(vet_plan *plan, const double *h_mu, const double *h_mv, const int32_t *h_ids, int n_users, int n_frames,
                        int window, int stride, double sigma_rad, int want_nss, double *h_stats, int64_t *h_counts, double *h_rows);

/* ---- hot path: TransitionEntropyAnalyzer.compute_entropy ------------------
 * (analyzers/transition_entropy.py:107-175 -> entropy_utils.py:213-332)
 * Output row r compares frame r (prior) with frame r+1 (current), r = 0..T-2.
 *   d_entropy  [T-1]
 *   d_pairs    [(T-1)*U*2]  (prior tile, current tile) of lattice 0, -1 if not in both (nullable)
 *   d_srccount [(T-1)*n_0]  users per source tile of lattice 0                          (nullable)
 *   d_common   [T-1]        users present in both frames                                (nullable)
 *   d_status   [2]          {bad, #rows without a common user}                          (nullable)
 *                           bad: as in vet_spatial_entropy                                        */
int vet_transition_entropy(vet_plan *plan, const double *d_mu, const double *d_mv,
                           int n_users, int n_frames,
                           double *d_entropy, int32_t *d_pairs, int32_t *d_srccount,
                           int32_t *d_common, int32_t *d_status, void *stream);
int vet_transition_entropy_ids(vet_plan *plan, const int32_t *d_ids, int n_users, int n_frames,
                               double *d_entropy, int32_t *d_pairs, int32_t *d_srccount,
                               int32_t *d_common, int32_t *d_status, void *stream);

/* ---- many videos, one launch ---------------------------------------------------
 * Short videos are launch-bound one call at a time (the reference's scale-out unit is "many short videos",
 * README.md:108-120); a batch shares one grid: the weighted table formulation (k_spatial_lut over the plan's fused
 * table), the nearest-tile / binned modes (k_spatial_u_lds, one launch per lattice) and transition mode
 * (k_transition_run, one launch per lattice, every video with its own workgroups).  Batches outside those kernels'
 * limits, and plans with vet_plan_set_fp64 on, run video by video inside the call.  Lattice 0's tile weights / source counts are not produced by the
 * batched forms.  Asynchronous on ``stream`` like vet_spatial_entropy. */
typedef struct vet_video {
    const double *d_mu, *d_mv;   /* [n_frames * n_users], frame-major */
    int n_users, n_frames;
    double *d_entropy;           /* [n_frames] */
    int32_t *d_assign;           /* [n_frames * n_users] or NULL */
    int32_t *d_present;          /* [n_frames] or NULL */
} vet_video;
int vet_spatial_entropy_batch(vet_plan *plan, int n_videos, const vet_video *videos, int32_t *d_status,
                              void *stream);
/* Same with concatenated host buffers (video v starts where video v-1 ends); synchronous. */
int vet_spatial_entropy_batch_host(vet_plan *plan, int n_videos, const int *n_users, const int *n_frames,
                                   const double *h_mu, const double *h_mv, double *h_entropy,
                                   int32_t *h_assign, int32_t *h_present);
/* Transition mode (TransitionEntropyAnalyzer.compute_entropy per video, analyzers/transition_entropy.py:107-175):
 * d_entropy [n_frames-1], d_assign = the (prior, current) tile pairs [(n_frames-1) * n_users * 2] or NULL,
 * d_present = users present in both frames [n_frames-1] or NULL; every video needs at least two frames. */
int vet_transition_entropy_batch(vet_plan *plan, int n_videos, const vet_video *videos, int32_t *d_status,
                                 void *stream);
int vet_transition_entropy_batch_host(vet_plan *plan, int n_videos, const int *n_users, const int *n_frames,
                                      const double *h_mu, const double *h_mv, double *h_entropy,
                                      int32_t *h_pairs, int32_t *h_common);

/* ---- host-buffer convenience: H2D, run, D2H, synchronous ------------------
 * Return VET_ERR_RANGE / VET_ERR_EMPTY when the status words are non-zero (outputs are still
 * written).  h_mu/h_mv may be NULL when h_ids is given and vice versa. */
int vet_spatial_entropy_host(vet_plan *plan, const double *h_mu, const double *h_mv,
                             const int32_t *h_ids, int n_users, int n_frames,
                             double *h_entropy, int32_t *h_assign, double *h_weights,
                             int32_t *h_present);
int vet_transition_entropy_host(vet_plan *plan, const double *h_mu, const double *h_mv,
                                const int32_t *h_ids, int n_users, int n_frames,
                                double *h_entropy, int32_t *h_pairs, int32_t *h_srccount,
                                int32_t *h_common);

/* ---- host-buffer runs whose optional outputs stay on the device -----------------------------
 * SpatialEntropyAnalyzer.compute_entropy returns per frame a dict of tile weights and a dict of tile
 * assignments (analyzers/spatial_entropy.py:152-163) which most callers never read (the CSV holds time and
 * entropy only, :216-219).  These variants bring back the entropy series (and the per-frame user counts)
 * and keep assign [T][U] i32 + weights [T][n_0] f64 (transition: pairs [(T-1)][U][2] i32 + srccount
 * [(T-1)][n_0] i32) in device memory owned by a vet_result, from which rows are fetched on demand.
 * Weighted spatial results hold the samples' direction ids [T][U] i32 instead of the weights when those are not larger
 * (U * 4 <= n_0 * 8 bytes per frame; otherwise the weight rows are stored) and compute the weight rows of a fetched block
 * when it is fetched (vet_plan_set_raw_weights: the reference's values, off the hot path; same bits as the eager output).
 * A result handle is returned also with VET_ERR_RANGE / VET_ERR_EMPTY.  vet_result_fetch may be called from several
 * threads on one result (fetches of lazily computed weight rows take turns on the result's staging buffer). */
typedef struct vet_result vet_result;
int vet_spatial_entropy_host_resident(vet_plan *plan, const double *h_mu, const double *h_mv,
                                      const int32_t *h_ids, int n_users, int n_frames,
                                      double *h_entropy, int32_t *h_present, vet_result **out);
int vet_transition_entropy_host_resident(vet_plan *plan, const double *h_mu, const double *h_mv,
                                         const int32_t *h_ids, int n_users, int n_frames,
                                         double *h_entropy, int32_t *h_common, vet_result **out);
/* which: 0 = assignments / pairs, 1 = weights / source counts; rows [row0, row0 + n_rows) -> h_dst */
int vet_result_fetch(vet_result *result, int which, int64_t row0, int64_t n_rows, void *h_dst);
int vet_result_free(vet_result *result);

/* ---- angular distances ------------------------------------------------------------------------
 * vector_angle_distance / find_angular_distances (utilities/entropy_utils.py:41-87) for m vectors x n tile centres:
 *   h_out[i*n + j] = arccos(clip(dot(v_i / |v_i|, t_j / |t_j|), -1, 1))   radians, [0, pi]
 * h_vectors [m*3] and h_tiles [n*3] are raw (not normalised) xyz, as Vector holds them; a zero-length vector gives NaN
 * (numpy's 0/0), no error.  Same arithmetic as the nearest-tile and weight kernels (find_nearest_tile is the first minimum
 * of a row of this matrix).  Synchronous. */
int vet_angular_distances(vet_ctx *ctx, const double *h_vectors, int64_t n_vectors, const double *h_tiles, int n_tiles,
                          double *h_out);

/* ---- tile boundary geometry of a Fibonacci tiling ---------------------------------------------
 * get_fb_tile_boundaries (utilities/data_utils.py:58-189): for every tile the boundary edges (pairs of points on
 * the unit sphere) in the order the reference appends them.  h_tiles [n*3] are the lattice Vectors as
 * generate_fibonacci_lattice returns them; h_edges [n][max_edges][2][3] (NaN padded), h_count [n] edges per tile.
 * VET_ERR_UNSUPPORTED when a tile has more than 32 neighbours within 1.7 x its nearest one or more than
 * max_edges edges.  Synchronous.  The corner walk and the spherical-excess areas built on the edges
 * (get_tile_corners :530-575, compute_spherical_polygon_area :657-678) stay on the host. */
int vet_fb_tile_boundaries(vet_ctx *ctx, const double *h_tiles, int n_tiles, int max_edges,
                           double *h_edges, int32_t *h_count);

/* ---- per-frame tile-attention heatmaps -------------------------------------------------------
 * The reference's tile-attention animation (PlotManager.update_frame / _get_color_from_intensity, create_animation,
 * utilities/visualization_utils.py:99-247) as uint8 RGB frames [n][H][W][3], C-contiguous, equirectangular: column c
 * covers longitude [-180 + 360c/W, -180 + 360(c+1)/W), row 0 is the top (lat +90), as video pixel coordinates.
 *   pixel -> tile: the nearest tile of the lattice (find_nearest_tile's first minimum, k_nearest_lut's arithmetic) to the
 *     unrounded Vector.from_spherical direction of the pixel centre; built once, by vet_heatmap_create;
 *   colour of a tile in frame t: _get_color_from_intensity(w / n) in FP64, w = tile_weights[t][tile] (+-0.0 = grey),
 *     n = users present (intensity 0 when n == 0): clip to [0, 1], red = i * (1 - 0.8) + 0.8, green = blue = 0.8 - i * 0.8,
 *     byte = floor(v * 255 + 0.5);
 *   markers (when samples are given): every present user paints a black square of side 2 * marker_radius + 1 centred on
 *     (row, col) = (min(py * H / video_height, H - 1), min(px * W / video_width, W - 1)), px = int(mu * video_width),
 *     py = int(mv * video_height) (integer division); columns wrap modulo W, rows clamp to [0, H); NaN = absent; a sample
 *     outside [0, 1] draws nothing and raises no error.
 * A heatmap belongs to its context (destroy it first) and, like the context, is used from one thread on one stream at a
 * time.  VET_ERR_INVALID: bad sizes, marker_radius outside [0, 16], a result of the other kind for the entry (spatial /
 * transition), a result of another device or lattice size; VET_ERR_UNSUPPORTED: a lattice larger than the map kernel's LDS tile cache (6783 tiles, the plans' own
 * limit). */
typedef struct vet_heatmap vet_heatmap;   /* W x H pixel -> tile map of one lattice, on one context's device */
int vet_heatmap_create(vet_ctx *ctx, const double *h_tiles /* [n_tiles*3] lattice Vectors */, int n_tiles, int width,
                       int height, int video_width, int video_height, int marker_radius, vet_heatmap **out);
int vet_heatmap_destroy(vet_heatmap *hm);
int vet_heatmap_read_map(vet_heatmap *hm, int32_t *h_map /* [H*W] */);
/* device pointers, asynchronous on `stream` (same stream convention as every other entry); d_rgb 4-byte aligned */
int vet_heatmap_render(vet_heatmap *hm, const double *d_weights /* [T][n_tiles] */, const int32_t *d_present /* [T] */,
                       const double *d_mu, const double *d_mv /* [T][U] or both NULL: no markers */,
                       int n_users, int n_frames, uint8_t *d_rgb /* [T][H][W][3] */, void *stream);
/* frames [row0, row0+n_rows) of a spatial vet_result -> host; synchronous.  The weight rows never leave the device (stored
 * rows are read in place; lazy ones are computed into the result's staging buffer); sub-blocks of frames alternate
 * between two pinned staging buffers so that the copy of one overlaps the kernels of the next: device memory does not
 * grow with n_rows. */
int vet_heatmap_render_result(vet_heatmap *hm, vet_result *r, const int32_t *h_present /* [n_rows] */,
                              const double *h_mu, const double *h_mv /* [n_rows][U] or NULL */, int n_users,
                              int64_t row0, int64_t n_rows, uint8_t *h_rgb);
/* Transition results (the reference's TransitionEntropyAnalyzer animation): frame r of the T-1 result rows is the pair
 * r -> r+1, coloured by _get_color_from_intensity(c / n) with c = srccount[r][tile] (the users present in both frames whose
 * frame-r nearest tile is this one; exact in FP64) and n = the users present in frame r (not the common-user count: a
 * user who leaves at r+1 counts in n and not in c); markers are the frame-r samples.  Same rules otherwise.
 * vet_heatmap_render_counts: device pointers, asynchronous on `stream`, as vet_heatmap_render. */
int vet_heatmap_render_counts(vet_heatmap *hm, const int32_t *d_counts /* [T][n_tiles] */, const int32_t *d_present /* [T] */,
                              const double *d_mu, const double *d_mv /* [T][U] or both NULL: no markers */,
                              int n_users, int n_frames, uint8_t *d_rgb /* [T][H][W][3] */, void *stream);
/* rows [row0, row0+n_rows) of a transition vet_result -> host; synchronous; the stored srccount rows are read in place,
 * through vet_heatmap_render_result's two-buffer pipeline.  h_present / h_mu / h_mv: frame r's users present and samples
 * for every row r of the range (the frame table's rows row0 .. row0+n_rows-1). */
int vet_heatmap_render_transition_result(vet_heatmap *hm, vet_result *r, const int32_t *h_present /* [n_rows] */,
                                         const double *h_mu, const double *h_mv /* [n_rows][U] or NULL */, int n_users,
                                         int64_t row0, int64_t n_rows, uint8_t *h_rgb);
/* Lat/lon cell heatmaps of a naive plan (the reference's NaiveSpatialEntropyAnalyzer; its own animation is commented out):
 * the same frames, colour rule, markers and marker radius, with these parts replaced:
 *   pixel -> cell: find_naive_tile_index (utilities/entropy_utils.py:362-381) of the pixel centre, FP64, C truncation:
 *     lon = (c + 0.5) / W * 360 - 180, lat = 90 - (r + 0.5) / H * 180,
 *     cell = (int)((lon + 180) / tile_width) * n_lat + (int)((lat + 90) / tile_height),  n_lat = 180 / tile_height + 1,
 *     out of (360 / tile_width + 1) * n_lat cells: the bin numbering (li * n_lat + lj) of the naive plan's LUT;
 *   colour of a cell in frame t: _get_color_from_intensity(count / present), count = the users whose sample falls in the
 *     cell through the plan's own quantiser (grid_dir) and LUT (the counts the frame's entropy is computed from), present
 *     = the users with a sample in frame t (intensity 0 when present == 0).  As the plan quantises: a sample at px = 0 has
 *     lon 0 (it counts in the lon-0 column, its marker is drawn at column 0); one at py = 0 (lat 90) or px = W (lon 180)
 *     counts in a cell of the extra row / column that no pixel centre maps to, so it dims the other cells and shows in
 *     none.  NaN = absent; a sample outside [0, 1] counts in neither count nor present and draws no marker (no error).
 * vet_heatmap_create_latlon: the cell map, built once; VET_ERR_INVALID for tile sizes <= 0 or not dividing 180 / 360 (the
 * rules of compute_naive_spatial_entropy) and the frame checks of vet_heatmap_create.  vet_heatmap_read_map gives its cells
 * (the device keeps slot lj * n_lon + li per pixel, so that a pixel row reads consecutive palette entries).
 * The binned entries take the samples [T][U] (frame-major, as every sample array) and a plan whose lattice 0 is binned on
 * a pixel grid, with the heatmap's cell count and video size (VET_ERR_INVALID otherwise, and for a heatmap of
 * vet_heatmap_create; the other render entries refuse a lat/lon heatmap).  Per frame one workgroup builds the cell histogram in
 * LDS, two 16-bit counts per word while n_users <= 65535, one u32 per cell above that: VET_ERR_UNSUPPORTED when those do
 * not fit the LDS (n_users > 65535 on grids of more than about 40 800 cells).  markers != 0: draw the viewport markers.
 * Frames run in chunks whose palette (n_cells u32 per frame) stays within 64 MiB.
 * vet_heatmap_render_binned: device pointers, asynchronous on `stream`; d_rgb 4-byte aligned.
 * vet_heatmap_render_binned_host: synchronous, through vet_heatmap_render_result's two-buffer pipeline, each block's
 * samples uploaded in it: device memory does not grow with n_frames. */
int vet_heatmap_create_latlon(vet_ctx *ctx, int tile_width, int tile_height, int width, int height, int video_width,
                              int video_height, int marker_radius, vet_heatmap **out);
int vet_heatmap_render_binned(vet_heatmap *hm, vet_plan *plan, const double *d_mu, const double *d_mv /* [T][U] */,
                              int n_users, int n_frames, int markers, uint8_t *d_rgb /* [T][H][W][3] */, void *stream);
int vet_heatmap_render_binned_host(vet_heatmap *hm, vet_plan *plan, const double *h_mu, const double *h_mv /* [T][U] */,
                                   int n_users, int n_frames, int markers, uint8_t *h_rgb /* [T][H][W][3] */);

/* ---- tilings drawn on the unit sphere --------------------------------------------------------
 * The scenes of the reference's pyvista tiling renders (save_*tiling_visualization_*, utilities/visualization_utils.py:
 * 306-674) as uint8 RGB frames [n][H][W][3], C-contiguous, row 0 at the top; pixel (row, col) has its centre at image
 * coordinates (X, Y) = (col + 0.5, row + 0.5).  All arithmetic is FP64.  This is the library's own frame definition (no
 * lighting, anti-aliasing or axes; not a pixel match of pyvista); tests/_tiling_oracle.py implements it in numpy.
 *   arcs: each (a, b) is drawn as the 49 chords between the spherical_interpolation points of a / |a| and b / |b| at
 *     t = np.linspace(0, 1, 50); an arc with coincident or antipodal ends (sin(theta) == 0 or clip(â.b̂) == -1: sin(pi) is
 *     1.2e-16 in FP64) draws nothing, and so does a chord with a non-finite end.  Duplicate arcs are allowed;
 *   camera (P, U, F) per frame: dist = |P - F|, d = (F - P) / dist, r = normalise(d x U), u = r x d, pixel size
 *     s = 2 dist sin(15 deg) / H (a parallel projection of a 30-degree view angle); X(p) = W/2 + (p - F).r / s,
 *     Y(p) = H/2 - (p - F).u / s; p is in front iff p.(-d) > 0.  dist == 0 or d x U == 0: VET_ERR_INVALID;
 *   line: the pixel centre is within distance <= 1 of a projected chord AB; tau = clamp((q - A).(B - A) / |B - A|^2, 0, 1)
 *     (0 when A == B), and the chord point P_i + tau (P_i+1 - P_i) decides front-line / back-line;
 *   point (centres): |X(c) - X_q| < 5 and |Y(c) - Y_q| < 5; c.(-d) > 0 decides front-point / back-point;
 *   disc: ((X_q - X0)^2 + (Y_q - Y0)^2) s^2 <= 1, (X0, Y0) the projection of the origin (the unit sphere);
 *   colour: under = back-point ? red : back-line ? black : background; pixel = front-point ? red : front-line ? black :
 *     disc ? blend(under) : under, blend(x) = floor(0.3 * 128 + 0.7 x + 0.5) per channel (grey 128 at opacity 0.3).
 * Frames are rendered in blocks of B = min(64, max(4, 32 MiB / (3 W H)) rounded down to a multiple of 4) frames, so device
 * memory does not grow with n_frames.  A tiling belongs to its context (destroy it first) and, like the context, is used
 * from one thread on one stream at a time.  VET_ERR_INVALID: a NULL argument, n_arcs, width, height or n_frames <= 0,
 * n_centres < 0, width or height > 16384, more than 2^22 arcs or 2^26 centres, an invalid camera. */
typedef struct vet_tiling vet_tiling;     /* the chord points (and centres) of one scene, on one context's device */
int vet_tiling_create(vet_ctx *ctx, const double *h_arcs /* [n_arcs][2][3] */, int n_arcs,
                      const double *h_centres /* [n_centres][3] or NULL */, int n_centres, int width, int height,
                      vet_tiling **out);
int vet_tiling_destroy(vet_tiling *tl);
/* h_cameras [n_frames][9] = (P, U, F) per frame, background [3] (RGB).  d_rgb: device, 4-byte aligned, [n][H][W][3];
 * asynchronous on `stream` (same stream convention as every other entry); the cameras are checked before any device work */
int vet_tiling_render(vet_tiling *tl, const double *h_cameras, int n_frames, const uint8_t *background, uint8_t *d_rgb,
                      void *stream);
/* the same frames to host memory h_rgb [n][H][W][3], synchronous, through two pinned staging blocks */
int vet_tiling_render_host(vet_tiling *tl, const double *h_cameras, int n_frames, const uint8_t *background,
                           uint8_t *h_rgb);

/* ---- host-side track loader (no GPU involved) -------------------------------------------
 * Replaces the per-file `pd.read_csv(filepath)` + column selection of process_viewport_data
 * (utilities/data_utils.py:305-316) for a whole directory: the files are parsed on n_threads host
 * threads (0 = all cores) into FP64 columns `time`, `2dmu`, `2dmv`, one entry per data row, NaN for
 * a missing value (rows are NOT dropped here; the caller applies dropna and the range checks).
 * The decimal conversion reproduces pandas' default C-engine converter bit for bit; a file that is
 * not plain unquoted numeric CSV gets status VET_CSV_FALLBACK and must be parsed by pandas. */
#define VET_CSV_OK 0
#define VET_CSV_FALLBACK 1   /* syntax outside the fast path: parse this file with pandas */
#define VET_CSV_IO 2         /* cannot open / read */
typedef struct vet_track {
    double *time, *mu, *mv;  /* malloc'ed by the library, n_rows each; release with vet_csv_free_tracks */
    int64_t n_rows;
    int status;              /* VET_CSV_* */
} vet_track;
int vet_csv_read_tracks(int n_files, const char *const *paths, vet_track *tracks, int n_threads);
void vet_csv_free_tracks(int n_files, vet_track *tracks);

#ifdef __cplusplus
}
#endif
#endif /* VET_H_ */
