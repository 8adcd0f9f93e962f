// vet_kernels.hpp — map of the gfx950 (MI355X, CDNA4) device code of the viewport -> tile -> entropy path.
//
// Kernels (wave = 64 lanes everywhere), by header and by the translation unit that launches them:
//   vet_plan.hip        vet_plan_kernels.hpp   k_grid_dirs      axis tables -> rounded + normalised direction per pixel (py,px)
//                                              k_unit_dirs      the same for an explicit direction table
//                                              k_nearest_lut    direction -> nearest lattice tile (np.argmin over arccos(dot):
//                                                               FP64 arg-max of the normalised dot, first minimum of the
//                                                               distance values), one LUT per lattice
//                                              k_angular_distances   vector_angle_distance for m vectors x n tile centres
//                       vet_weight_table.hpp   k_row_stats      exact rows -> error bounds of the integer formulations
//                                              k_wtab           direction -> ELL row of (tile, FoV weight), ocml acos / pow
//                                              k_fuse_shifts, k_dirrec   fused-row shifts, per-direction records
//                                              k_wexact         direction -> ELL row of (tile, exact FP64 weight) of lattice k:
//                                                               the rows the weights pass (lattice 0) and k_spatial_dtable gather
//                       vet_geometry.hpp       k_fb_boundaries  tile boundary edges of a Fibonacci tiling
//   vet_spatial.hip     vet_spatial_lut.hpp    k_spatial_lut    table formulation: per frame, samples -> direction ids ->
//                                                               gather of the users' rows into 64-bit integer (or FP64) LDS
//                                                               histograms (all lattices in one launch) -> Shannon entropy
//                       vet_spatial_sweep.hpp  k_spatial_w      sweep formulations (few samples per plan): lane = tile, FP64
//                                                               cone test per (user, tile), full-wave weight evaluation
//                       vet_weights_pass.hpp   k_weights_gather the tile_weights output (values at the reference's precision):
//                                                               per frame, the users' exact weight rows summed in column
//                                                               order (off the hot path; k_spatial_w<PRECISE> in weights-only
//                                                               mode where the exact rows do not fit the device)
//                       vet_spatial_dtable.hpp k_spatial_dtable dtable formulation (fp64 plans): the weights pass's gather over the
//                                                               exact FP64 rows of every lattice + the reference's entropy in FP64
//                       vet_spatial_u.hpp      k_spatial_u_lds  nearest-tile (unweighted) and naive lat/lon-grid mode:
//                                                               persistent stream with the nearest LUT in LDS (HBM-bound)
//                                              k_spatial_u      generic fallback (LUT gathered from global memory)
//   vet_window.hip      (in the unit)          k_window_tiles   per frame: tile / bin of every sample, present count
//                                              k_window_entropy_w, k_window_entropy_c   sliding windows of frames pooled into one
//                                                               histogram per row (weighted: the frames' exact FP64 sums added in
//                                                               frame order; counts: add entering, subtract leaving frames) ->
//                                                               the reference's entropy of the pooled histogram
//                                              k_window_transition   sliding windows of frame pairs: the pooled (pair, user)
//                                                               transitions of a row walked by k_transition_big's row algorithm
//   vet_window_divergence.hip  (in the unit)   k_window_hist_w, k_window_hist_c   the rows' pooled histograms (vet_window_hist.hpp:
//                                                               k_window_entropy's sums), their totals and NaN flags, per row chunk
//                                              k_window_divergence   one thread per (row, lag): Jensen-Shannon divergence of rows r
//                                                               and r + l in the overlap form, histograms staged through LDS
//   vet_coverage.hip    (in the unit)          k_coverage_rank  one workgroup per row: lattice 0's pooled histogram sorted in LDS (vet_rank.hpp),
//                                                               the sequential running sum in rank order, the top-k tile counts that hold
//                                                               the asked shares of the mass, the rank of every tile
//                                              k_coverage_hits  one wave per (row, lag): the share of row r + l's mass on row r's top-k tiles
//   vet_markov.hip      (in the unit)          k_markov_rows    one workgroup per row of up to 32768 candidate samples: the keys source * n +
//                                                               destination sorted in LDS (the unit's own walk of a bitonic network), run lengths = pair counts ->
//                                                               entropy rate, stationary / destination entropy, mutual information,
//                                                               stay share; the dense transition matrix by plain stores
//                                              k_markov_count   longer rows: the same sort and run lengths per chunk of 32768 samples,
//                                                               one global integer atomicAdd per run into the row's dense matrix
//                                              k_markov_cells   one workgroup per row: the dense matrix walked in index order -> the
//                                                               same five statistics
//   vet_motion.hip      (in the unit)          k_motion_angles  one FP64 angle per (frame pair, viewer): two unit vectors gathered from the
//                                                               direction table, fused dot, clip, acos; +0.0 for the same Vector
//                                              k_motion_wave    one wave per row of up to 64 angles: sums by wave_sum, the bit patterns
//                                                               sorted across the lanes by shuffles
//                                              k_motion_rows    one workgroup per row of up to 16384 angles: block-ordered sums, the bit
//                                                               patterns sorted in LDS, quantiles between exact order statistics
//                                              k_motion_chunk   longer rows: the same sums per chunk of 16384, and a pass of the
//                                                               radix selection (the next 8-bit digit under the wanted prefixes)
//                                              k_motion_select  one wave per row: partial sums in block order, each wanted rank
//                                                               narrowed to its digit; after eight passes the exact values
//   vet_dispersion.hip  (in the unit)          k_dispersion_pairs   workgroup = (frame, 256 viewers): the frame's unit vectors staged in LDS,
//                                                               every thread walks its viewer's partners in ascending order (fused
//                                                               dot, clip, acos; an LDS broadcast per partner): sum, nearest, farthest,
//                                                               counts per (frame, viewer), the frame's edge histogram
//                                              k_dispersion_chunk   16 blocks of 1024 positions of a row: block-ordered partial sums,
//                                                               the row's integers by integer atomics
//                                              k_dispersion_finish  one wave per row: the blocks in order, the frames' histograms added
//   vet_cluster.hip     (in the unit)          k_cluster_ids    the direction ids of the samples, frame-major
//                                              k_cluster_links  workgroup = (row, 256 viewers, a tile of partners): the partners' unit
//                                                               vectors of a chunk of frames staged in LDS, every lane counts for 8
//                                                               partners the frames both are in and those in which they are near
//                                                               (fused dot against a cosine; no acos), one ballot per partner = a
//                                                               64-bit word of the row's LINKED matrix
//                                              k_cluster_components  one workgroup per row: label propagation over the link bits with
//                                                               pointer jumping in LDS, the roots ranked, sizes, the sorted
//                                                               (size, label) records, the partition entropy, the centroids
//   vet_fixation.hip    (in the unit)          k_fix_runs       one workgroup per viewer walks the frames in order in chunks of 1024: run
//                                                               starts by a max-scan (lanes, waves, a carry between chunks), the
//                                                               length of every run written at its start
//                                              k_fix_offsets    the exclusive prefix of the viewers' event counts
//                                              k_fix_labels     the same walk: every sample's label, the event list by a sum-scan
//                                              k_fix_frames     pooled layout: a frame's totals over 64 viewers, integer atomics
//                                              k_fix_rows       a wave or a workgroup per row sums the row's frames
//                                              k_fix_centroids  one thread per listed event: its unit vectors in frame order
//   vet_saliency.hip    (in the unit)          k_saliency_ids   the pooled layout's direction ids, frame-major (per viewer: k_user_dirs)
//                                              (shared by the kernels below, written once: sal_walk — the density of a list at a
//                                                               direction; sal_rule — the block-ordered summation rule of a workgroup, and
//                                                               cg_wave_rule, the same by one wave; sal_pixel_terms — the comparison terms)
//                                              k_saliency_sort  one workgroup per row of up to 4096 positions: LDS sort of the ids, the
//                                                               distinct ids in ascending order with their run lengths
//                                              k_saliency_count, k_saliency_compact   longer rows: dense integer counts per direction,
//                                                               compacted in ascending id by one workgroup per row
//                                              k_saliency_map   workgroup = (row, 256 pixels): the row's list staged in LDS in tiles of
//                                                               1024 entries, S = fma(m, exp(kappa (c - 1)), S) per pixel in a register (sal_walk)
//                                              k_saliency_rows  one workgroup per row: mass, peak, entropy and area of the written map
//                                              k_saliency_mask  the similarity call: the ids once more per audience, the others' samples -1
//                                              k_saliency_points  workgroup = (row, 256 entries of one audience's list, direction): the
//                                                               other audience's density at the entries' directions by sal_walk
//                                              k_saliency_compare  one workgroup per row: the masses, CC, SIM, JSD, both KL and both NSS
//                                                               of the two audiences' maps by sal_rule over sal_pixel_terms
//                                              k_congruency_points  the congruency call: workgroup = (row, 256 queries), a query = one entry
//                                                               of one viewer's own list; the pooled list in LDS tiles with its ids, the
//                                                               viewer's own multiplicity taken off on an id match (leave-one-out)
//                                              k_congruency_users  one wave per (row, viewer): the own-entry sums by the block-ordered rule
//                                              k_congruency_rows  one workgroup per row: Q, every viewer's lift, information gain and NSS,
//                                                               the row's means over the scored viewers
//                                              k_score_sort     the scoring call: workgroup = (map row, predicted map): the row's W bit patterns
//                                                               sorted in LDS (non-negative doubles order as their bits), a sorted copy
//                                              k_score_points   workgroup = (row, 256 list entries): the predicted map at the entry's direction
//                                                               (bilinear), its rank in every sorted map row by two binary searches in LDS
//                                              k_score_rows     one workgroup per row: mass and variance of the prediction, AUC, NSS and
//                                                               information gain from the list sums, CC, SIM, JSD, KL against the audience's map (sal_pixel_terms)
//   vet_crowd.hip      (in the unit)          k_crowd_logp     log2 of the pooled proportions of a chunk's rows, once per row and tile
//                                              k_crowd_w, k_crowd_c   one workgroup per (row, viewer): k_user_entropy_w/_c's walk in LDS, then
//                                                               W_u, S(h_u) and the viewer's KL divergence from the pooled row in one wave
//                                              k_crowd_rows     one wave per row: pooled, within and between
//   vet_bootstrap.hip   (in the unit)          k_bootstrap_counts   how often each replicate's draw picked each viewer, u16 [B][U]
//                                              k_bootstrap_zero_keys   flagged (row, viewer) slots: the keys whose value is 0.0, as bits
//                                              k_bootstrap_gemm one workgroup per (row, 16 replicates): counts x per-viewer histograms
//                                                               (k_user_hist_w/_c's) on the FP64 matrix unit into LDS, then the
//                                                               row calls' entropy epilogue per replicate
//                                              k_bootstrap_summary   one workgroup per row: the finite replicates sorted in LDS ->
//                                                               mean, sd and the two quantiles
//   vet_group.hip       (in the unit)          k_group_labels   one workgroup per permutation: the keys of the included viewers sorted in
//                                                               LDS -> labels u8 [P + 1][U] (row 0 the observed groups)
//                                              k_group_gemm     one workgroup per (row, 8 labellings): 0/1 group masks x per-viewer
//                                                               histograms on the FP64 matrix unit, A sums in rows 0-7 and B sums
//                                                               in rows 8-15 of the tile, into LDS; then W and S of A, B and A + B
//                                                               and the Jensen-Shannon divergence per labelling
//                                              k_group_samples  the observed audiences' present samples per row
//                                              k_group_maxnull  one thread per permutation: its largest finite value over the rows
//                                              k_group_summary  one workgroup per row: p-values, mean and the sorted quantile of the null
//                       vet_rank.hpp           lds_bitonic_sort, lerp_quantile: shared by vet_bootstrap.hip, vet_group.hip and vet_coverage.hip
//   vet_transition.hip  vet_transition.hpp     k_transition_run per frame pair: (prior tile, current tile) pairs -> bucket
//                                                               statistics in LDS -> transition entropy; persistent workgroups
//                                              k_transition_big more than 4096 users: the bucket hash in LDS, the row cut into
//                                                               ranges of source tiles whose buckets fit it
//                                              k_transition_any fallback for lattices of thousands of tiles (hash in global scratch)
//   vet_heatmap.hip     (in the unit)          k_heatmap_map    pixel -> nearest tile of a lattice (nearest_tile, as k_nearest_lut)
//                                              k_heatmap_palette, k_heatmap_fill, k_heatmap_markers   per-frame tile-attention
//                                                               RGB frames: palette per (frame, tile), streamed gather-store
//                                                               of the pixels, viewport markers
//   vet_tiling.hip      (in the unit)          k_tiling_chords, k_tiling_splat, k_tiling_compose   a tiling drawn on the unit
//                                                               sphere: arcs -> slerp points, per-pixel line / point flags,
//                                                               streamed RGB compose
//   (several units)     vet_finalize.hpp       k_log2_table, k_finalize*   log2(k) table; mean over a plan's lattices
// Shared, kernel-free headers: vet_layout.hpp (table / histogram layout constants), vet_common.hpp (wave helpers, the
// sample -> direction-id quantiser), vet_weights.hpp (FoV weight, weighted frame entropy), vet_window_hist.hpp (a window's pooled sums and counts),
// vet_divergence.hpp (x log2 x, the reference's NaN test of a key), vet_row_hist.hpp (a finished row histogram in one wave: total,
// entropy, NaN flag, the epilogue over counts — one copy for the per-viewer and the windowed units), vet_host.hpp (host state).
// vet_user_dirs.hpp holds k_user_dirs (stage 1 of the per-viewer units) and the two walks that build a viewer's row histogram.
//
// No MFMA: there is no dense contraction on this path.  Reference citations are relative to
// /root/reference/src/viewport_entropy_toolkit/.  This header is documentation; the units include what they launch.
#pragma once
