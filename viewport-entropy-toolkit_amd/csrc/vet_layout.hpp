// vet_layout.hpp — table and histogram layout constants shared by the host code and the kernels (no kernels here)
// Part of the gfx950 device code of the viewport -> tile -> entropy path (see vet_kernels.hpp for the map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vet {

constexpr int WAVE = 64;
constexpr int MAX_LATTICES = 8;

// direction weight table (vet_weight_table.hpp)
constexpr int TAB_X = 16;                                // histogram unit 2^-(32+TAB_X): sums of < 2^16 weights <= 1 fit 64 bits
constexpr uint32_t MARKER_BITS = 0x80000000u;            // -0.0f: FP-table entry of an in-FoV tile without an FP32 value
constexpr int ROW_BITS = 19;                             // set key = row (19 bits) | mirror flag; slot = key << 12 | count
constexpr uint32_t ROW_MASK = (1u << ROW_BITS) - 1;
constexpr unsigned DEDUP_MAX_DIRS = (1u << ROW_BITS) - 1;
constexpr int DEDUP_MIN_USERS = 128;                     // frames of fewer users run the table kernel without the set (LutParams)

// Capped rows (ensure_wtab; integer one-lattice tables with 16-lane rows).  Main rows are `cap` slots = cap / ROW_BLOCK whole
// blocks, which the table kernel walks with a fixed, unrolled trip count; the few rows (at most 1 in 32) that are longer keep
// their entries beyond `cap` in one ROW_BLOCK-slot block of a side table, found through ovf_of_row[row] by the rows whose meta
// word has META_OVERFLOW set (the length of a capped row is at most cap <= 192: bit 15 of the length field is free, and the
// record of k_dirrec carries it).  The fixed-trip kernels exist for 1..MAX_CAP_BLOCKS blocks.
constexpr int ROW_BLOCK = 64;
constexpr int MAX_CAP_BLOCKS = 3;
constexpr uint32_t META_OVERFLOW = 1u << 15;
constexpr uint32_t NO_OVERFLOW = 0xFFFFFFFFu;

// Compact direction record of the capped kernels (k_dirrec32; k_spatial_lut<REC32>): a capped row has no length to carry, so
// what a sample needs fits one word —  row | mirrored << 15 | nearest tile << 16 | -shift << 26 | continues in the side
// table << 31  (shift = the row's block-floating-point exponent in [-TAB_X, 0]: the meta word holds TAB_X + shift).  Built
// beside the 8-byte record where rows + 1 <= 2^REC32_ROW_BITS and the lattice has at most 2^REC32_TILE_BITS tiles.
constexpr int REC32_ROW_BITS = 15;
constexpr int REC32_TILE_BITS = 10;
constexpr int REC32_SHIFT_BITS = 5;
constexpr uint32_t REC32_ROW_MASK = (1u << REC32_ROW_BITS) - 1;
constexpr uint32_t REC32_KEY_MASK = (1u << (REC32_ROW_BITS + 1)) - 1;       // row | mirrored: the set's key
constexpr int REC32_TILE_POS = REC32_ROW_BITS + 1;
constexpr int REC32_SHIFT_POS = REC32_TILE_POS + REC32_TILE_BITS;
constexpr uint32_t REC32_OVERFLOW = 1u << 31;
constexpr uint32_t REC32_AUX_MASK = ~((1u << REC32_SHIFT_POS) - 1);          // -shift and the overflow bit, as they sit
static_assert(REC32_SHIFT_POS + REC32_SHIFT_BITS == 31, "row, mirror, tile, shift and the overflow bit fill 32 bits");
static_assert(TAB_X < (1 << REC32_SHIFT_BITS), "-shift in [0, TAB_X] fits its field");
static_assert(REC32_ROW_BITS <= ROW_BITS, "a compact row is a row of the set");
// The row list of the REC32 kernels, one word per row and no meta word:  left shift (TAB_X + shift) in bits 0..4 |
// multiplicity - 1 (chunks of at most 2048 users) << 5 | row << 16 | mirrored << 31.  Rows listed one per user (no set) have
// multiplicity 1: bit 5 then marks "continues in the side table" until the overflow list is made.
constexpr int WALK32_CNT_POS = 5, WALK32_CNT_BITS = 11, WALK32_ROW_POS = 16;
constexpr int REC32_MAX_CHUNK = 1 << WALK32_CNT_BITS;
constexpr uint32_t WALK32_OVF_TMP = 1u << WALK32_CNT_POS;
static_assert(WALK32_CNT_POS + WALK32_CNT_BITS == WALK32_ROW_POS && WALK32_ROW_POS + REC32_ROW_BITS + 1 == 32, "walk word");
static_assert(TAB_X < (1 << WALK32_CNT_POS), "the left shift fits below the multiplicity");
// Bucket-ordered row lists that start at bucket b0 and wrap around (k_spatial_lut<LB > 0>): the list position `pos` of the
// ascending order moves to pos - p0, plus cnt where that is negative — p0 = the first position of bucket b0, cnt = the list's
// entries, 0 <= pos, p0 <= cnt.  A bijection of 0 .. cnt - 1 that keeps the order on either side of the wrap.  p0 is the first
// position of a bucket, so no bucket straddles it and rotated(first + rank) = rotated(first) + rank for every entry of a
// bucket: the kernel rotates the buckets' first positions, once per bucket, and places the words as before.
__host__ __device__ __forceinline__ uint32_t lut_rotated(uint32_t pos, uint32_t p0, uint32_t cnt) {
    const int32_t d = (int32_t)pos - (int32_t)p0;
    return (uint32_t)(d < 0 ? d + (int32_t)cnt : d);
}
// The sweep that tells a starting workgroup its b0: the 100 MHz wall clock passes all buckets once per 2^13 ticks = 82 us,
// about the time a frame of ~700 distinct rows takes to walk its list (config 3: ~60 us).  Periods of 45 to 90 us measured
// within 0.8 % of each other (profiles/phase_walk/components.txt): what counts is that walks that start together start at
// the same bucket, so a power of two, which makes b0 one shift of the clock.
constexpr int LUT_SWEEP_TICKS_LOG2 = 13;

// entries of a frame's overflow list (LDS): with the set of distinct rows at most one per (overflow row, mirrored) — fewer than
// DEDUP_MIN_USERS where a small video of a batch runs without the set —, otherwise one per user; never more than the chunk
__host__ __device__ __forceinline__ int lut_ovf_slots(int UC, int n_ovf, bool dedup) {
    if (n_ovf <= 0) return 0;
    const int most = dedup ? (2 * n_ovf > DEDUP_MIN_USERS ? 2 * n_ovf : DEDUP_MIN_USERS) : UC;
    return most < UC ? most : UC;
}

// ------------------------------------------------------------------------------------------
// Fused histogram layout.  The plan's K lattices (analyzers/spatial_entropy.py:142-156 loops over
// them per frame) share ONE histogram of N = Nr + 4K slots, Nr = 2 * (Hs + K), Hs = sum_k floor(n_k / 2):
//     [ 2K spare slots | first halves of lattices 0..K-1 | K centre slots | K mirrored centre slots |
//       second halves, reversed | 2K spare slots ]
// laid out so that the ONE reflection pos -> N-1-pos maps every lattice onto itself the way the Fibonacci
// lattice's mirror symmetry (x,y,z) -> (x,-y,-z) does (tile i <-> tile n_k-1-i, see ensure_alias): a direction
// and its mirror image then share one fused table row, the mirrored one adding into N-1-pos.  The centre tile
// of an odd lattice is its own mirror image; it owns two slots and the epilogue adds them.
// A distinct direction of a frame costs ONE row walk (one length word, one set-up) whatever K is, and the
// short rows of small lattices share cache lines with the others (config 4, 51+101+201 tiles: 88 entries =
// 5 lines instead of 3 rows x 3 lines + 2 meta words).
// ------------------------------------------------------------------------------------------
struct FusedLayout {
    int K;
    int n[MAX_LATTICES];        // tiles per lattice
    int off[MAX_LATTICES];      // slot of tile 0 of lattice k = 2K + sum_{j<k} floor(n_j / 2)
    int Hs, N;                  // N = 2 * (Hs + K) + 4K
    int CF;                     // 64-tile chunks per frame = sum_k ceil(n_k / 64)
    double hmax[MAX_LATTICES];
};
__host__ __device__ __forceinline__ int fused_pos(const FusedLayout& L, int k, int i) {
    const int h = L.n[k] >> 1;
    if (i < h) return L.off[k] + i;
    if (i >= L.n[k] - h) return L.N - 1 - (L.off[k] + (L.n[k] - 1 - i));
    return 2 * L.K + L.Hs + k;
}

// One lattice's exact weight rows as the gathers see them (k_wexact output; rows = the plan's canonical directions); the host
// fills it with exact_rows_arg (vet_host.hpp)
struct ExactRows {
    const uint16_t* idx;        // [R][stride]
    const double* w;            // [R][stride]
    const uint32_t* len;        // [R]
    int stride, n;
};

}  // namespace vet
