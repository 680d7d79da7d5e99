// Plane-gradient scatter (autograd of the 12 grid_sample calls of reference src/networks/decoders.py:79-81):
// spatially ordered ray bundles + a per-workgroup sort of the bundle's samples by texel cell + register run-merge.
//
// Why: on the bench workload (room0, 4096 x 64) the 262144 samples make 12.6 M texel contributions but touch only
// ~36 k distinct texels (4.6 MB of the 27 MB of planes), because all rays of a frame leave from one camera centre.
// Global float atomics run at ~1.3 TB/s of added bytes chip-wide (MI355X_MICROARCH.md, "Global float atomics"), so
// the cost of the scatter is the number of 256-B atomic wave-instructions that reach memory (tools/sim_scatter.py):
//      unmerged                                             6.29 M  -> 1.24 ms at the atomic rate
//      v1: run-merge along each ray (scatter_kernel)         2.19 M  -> 0.43 ms   (measured 0.81 ms: hot texels contend)
//      bundles of ~16 rays of similar direction, merged      ~0.3 M  -> 0.06 ms
// An LDS hash table of texel accumulators fed with ds_add_f32 reached that atomic count but ran 2.2 ms: one dependent
// global load + two LDS float atomics per sample and plane, at the 1-2 workgroups per CU the tables leave room for.
// What is built instead needs no LDS atomics at all:
//
// ray_order_kernel    sorts rays by a Morton key of their direction (and origin cell): neighbours in the order are rays
//                     through neighbouring pixels of one camera, which cross the same texels for most of their length.
// scatter_sort_kernel one workgroup = one bundle of consecutive rays in that order x one plane.  It (1) computes the
//                     bilinear cell of each of the bundle's <= 1024 samples, (2) sorts the samples by cell in LDS
//                     (bitonic network), (3) gives each wave a contiguous quarter of the sorted list to walk with
//                     lane = (x-corner, channel): consecutive entries of one cell are summed in two registers (rows
//                     y0, y1) and each cell is written once with two 256-B-shaped float atomics.
#include <mutex>
#include <type_traits>
#include "eslam_decode_tile.h"
#include "eslam_dec_reduce.h"
#include "eslam_ray_order_dev.h"

typedef float float2_t __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------
// ray ordering (the body: eslam_ray_order_dev.h, shared with step_front_kernel)
// ---------------------------------------------------------------------------------------------------------
// One launch, two independent roles chosen by the block number: blocks [0, n_order = chunks * ESLAM_RAY_ORDERS) order the rays
// (block b: chunk b / ESLAM_RAY_ORDERS, orientation b % ESLAM_RAY_ORDERS - the lowest numbers, so that they are placed first: they
// are the long ones), the blocks behind them zero clear_words floats at `clear` (16-byte aligned; the iteration's plane-gradient
// buffer) with 16-byte stores.  A replayed hipGraph pays ~3 us per node whatever its size (shard_prologue_kernel), and a memset
// node in front of the order held the order back by the memset's whole length.
__global__ __launch_bounds__(1024) void ray_order_kernel(const float* __restrict__ rays_o,
                                                         const float* __restrict__ rays_d, int R,
                                                         int* __restrict__ perm, int key_bits, const int n_order,
                                                         float* __restrict__ clear, const long long clear_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned hist[];       // ray_order_lds_bytes(key_bits): counters, then sorted ids
    if ((int)blockIdx.x >= n_order) {
        ray_clear_block(clear, clear_words, (int)blockIdx.x - n_order, (int)gridDim.x - n_order);
        return;
    }
    ray_order_block(rays_o, rays_d, R, perm, key_bits, (int)blockIdx.x, hist);
}

// ---------------------------------------------------------------------------------------------------------
// bundle scatter
// ---------------------------------------------------------------------------------------------------------
// NT = 512 threads per workgroup, BM = SPT*NT samples per workgroup (power of two).
//   (Round 2 had the kernel's two halves - cells + sort / walk - as separately launchable phases, the first one beside the
//   forward kernel on a side stream: 0.369 vs 0.323 ms per step, DESIGN.md section 10.  Removed in round 3.)
//   DET (ESLAM_DETERMINISTIC=1): the sums of a cell are formed in 64-bit fixed point (2^-44 units: integer adds commute, so
//   neither the arbitrary order of the counting sort's tickets inside a cell, nor the order in which workgroups' atomics
//   reach a texel, nor the ray order itself can change a bit of the result) and added to an int64 shadow of the gradient
//   planes; scatter_fixed_to_float_kernel then adds the shadow to the float gradients and clears it.
#define FIX_SCALE 17592186044416.0f                  // 2^44: resolution 5.7e-14
#define FIX_LIMIT 262144.0f                          // |one contribution| < 2^18: 2^62 in fixed point; a texel's SUM wraps beyond
                                                     // 2^63 / 2^44 = 5.2e5 - contributions past the limit poison the gradient (NaN)
// What is and is not detected: a CONTRIBUTION that is NaN / Inf or at least FIX_LIMIT in magnitude sets det_bad in the lane that
// holds it, and the flush of that lane's sums adds NaN to exactly the texels those sums go to (along a run of minor-axis
// adjacent cells det_bad moves to the lower half-wave together with the carried column, so it never reaches a texel the
// contribution did not touch).  A texel's SUM that leaves +-5.2e5 while every contribution is in range wraps undetected.
struct ShadowOff { int64_t o[NPL]; };
// GZ (the rank-16 path, see mlp_bwd_kernel): g_feat holds gz[2][N][16], the gradient at the decoders' first hidden layer, and
//   the features' gradient W1^T . g_z1 is never formed per sample.  The walk sums w * g_z1 per cell in the 16-wide space - four
//   sorted entries per step, lane (slot = lane >> 4, j = lane & 15) with the entry's four corner sums, one 64-byte row per entry
//   shared by the six planes of a decoder - and the flush adds the slots and multiplies the cell's 2 x 2 x 16 sums by the plane's
//   [16, 32] slice of W1 (LDS, staged once per workgroup) before the same two atomics per lane (hx, c).  tests/rank16_ref.py
//   states what is computed, tests/quad_walk_ref.py restates the walk's bookkeeping in numpy.
constexpr int SC_NT = 512;
constexpr int GZ_WP = 20;                           // pitch (floats) of the W1 slice's rows [c][j]: 16-byte aligned, conflict-free
// PAIR (rank-16 path): a workgroup may serve the two planes pi and pi + 6 of one (orientation, level) - the SDF decoder's and the
//   colour decoder's.  They bundle the same rays, and where they agree in resolution and strides (the host checks it pair by
//   pair: the reference's default colour planes are twice as fine at the fine level, so only the coarse pairs agree there) cells,
//   bounding box, sort and the sorted records are the same entry for entry: phases (1) and (2) run once and the walk runs twice
//   over the records that are still in LDS, per pass with the decoder's half of gz, its gradient plane and its slice of W1
//   (restaged between the passes: both slices do not fit beside the records at three workgroups per CU).  The grid runs over a
//   work list per bundle instead of the 12 planes: the planes left single in front (the fine planes: most cells, most flushes,
//   the longest workgroups), the agreeing pairs (two short walks over few cells) behind them, where they fill the grid's tail.  The
//   list arrives in `shoff`, which only the fixed-point instantiations use otherwise: o[w] = plane | walks << 4, and its length
//   in o[0] << 8.
template <bool RENDER, bool DET, int SPT = 4, bool GZ = false, bool PAIR = false>
__global__ __launch_bounds__(SC_NT) __attribute__((amdgpu_waves_per_eu(PAIR ? (SPT == 4 ? 6 : 8) : 2))) void scatter_sort_kernel(const PlaneSet planes, const Bound bnd,
                                                          const float* __restrict__ rays_o,
                                                          const float* __restrict__ rays_d,
                                                          const float* __restrict__ z_vals,     // RENDER ? [R,S] : pts [N,3]
                                                          const int* __restrict__ perm, int R, int S,
                                                          const float* __restrict__ g_feat, int bundle, int nbundles,
                                                          long long* __restrict__ shadow,
                                                          const ShadowOff shoff, const DecReduceArgs red, const int red_blocks,
                                                          const float* __restrict__ gz_w1_sdf, const float* __restrict__ gz_w1_rgb) {
    constexpr int NT = SC_NT;
    static_assert(!GZ || (RENDER && !DET), "GZ: the float render path only");
    static_assert(!PAIR || GZ, "PAIR: the rank-16 path only");
    const int NPLW = PAIR ? (int)(shoff.o[0] >> 8) : NPL;   // planes (PAIR: entries of the work list) the grid runs over
    constexpr int BM = SPT * NT;                       // SPT samples per thread in the cell / sort phases
    constexpr int CH = WAVE * SPT;                     // sorted entries a wave walks
    static_assert(SPT == 2 || SPT == 4, "samples per thread");
    constexpr int SLOT_BITS = (BM == 1024) ? 10 : 11;
    constexpr unsigned SLOT_MASK = BM - 1;
    static_assert(BM == 1024 || BM == 2048, "bundle size");
    // 6*BM words (48 KB at BM = 2048; 3 workgroups per CU).  Layout the walk reads, records in SORTED order:
    //   sw    [BM] float4  bilinear weights of the entry for lane halves hx = 0 / 1 and rows 0 / 1:
    //                      ((1-tm)(1-tM), (1-tm)tM, tm(1-tM), tm tM) - a lane reads its (row 0, row 1) pair with one
    //                      ds_read_b64, so the per-entry VALU work of the walk is ONE packed FMA
    //   sxy   [BM] byte offset of texel (x0,y0) << 2 | minor-axis step flag | major flag << 1; 0xFFFFFFFF = padding
    //   sgrow [BM] row of g_feat (global point index)
    // The sort phases use the same memory differently (see below).
    __shared__ __attribute__((aligned(16))) unsigned lds_raw[6 * BM];
    // GZ: + 2560 B for the plane's slice of W1 as [c][j] and + 2048 B of wave-private exchange (a cell's 64 sums): 53 760 B at
    // BM = 2048, three workgroups per CU as before
    __shared__ __attribute__((aligned(16))) float gz_w[GZ ? ESLAM_C_DIM * GZ_WP : 4];
    __shared__ __attribute__((aligned(16))) float gz_a[GZ ? NT : 4];
    float4_t* const sw = (float4_t*)lds_raw;
    unsigned* const sxy = lds_raw + 4 * BM;
    int* const sgrow = (int*)(lds_raw + 5 * BM);
    unsigned* const cnt = lds_raw;                     // counting sort: 4*BM packed 16-bit counters (dead before sw is written)
    unsigned* const swsum = lds_raw + 2 * BM;          // counting sort: per-wave totals of the scan
    int* const sbox = (int*)(lds_raw + 2 * BM + 64);   // bounding box of the bundle's cells (registers before sw is written)
    // bitonic fallback (boxes too large for the counters): keys + slot-indexed temporaries, permuted into the layout above
    unsigned* const skey = lds_raw;                    // (cell << SLOT_BITS) | local sample slot
    unsigned* const txy = lds_raw + BM;
    float* const ttm = (float*)(lds_raw + 2 * BM + 128);   // after sbox / swsum
    float* const ttM = (float*)(lds_raw + 3 * BM + 128);
    int* const trow = (int*)(lds_raw + 4 * BM + 128);
    constexpr unsigned PAD_XY = 0xFFFFFFFFu;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hx = lane >> 5, c = lane & 31;   // hx: corner along the MINOR axis

    // The first red_blocks workgroups (a multiple of 8) are not scatter workgroups:
    // they sum the decoder-gradient slabs of the decoder backward that ran just before (eslam_dec_reduce.h), beside the
    // scatter's first workgroups instead of as a launch of their own in front of them.
    if (red_blocks > 0 && (int)blockIdx.x < red_blocks) {
        if ((int)blockIdx.x < 2 * DEC_RED_COLBLOCKS)
            dec_grad_reduce_block<NT>(red, blockIdx.x % DEC_RED_COLBLOCKS, blockIdx.x / DEC_RED_COLBLOCKS, (float*)lds_raw);
        return;
    }
    const int bid = (int)blockIdx.x - red_blocks;
    // Workgroup -> (bundle, plane), 1-D grid, chosen on the device: plane-major for a WIDE fan of rays from one origin,
    // bundle-major otherwise.  Measured (profiles/r03/l_*, one ray order per orientation; the parent of the commit that removed
    // the other layouts reproduces them):
    //   bundle-major: the 12 planes of bundle 0, then of bundle 1, ...  The four planes of an orientation bundle the same rays
    //     and read the four 128-byte segments of the same feature-gradient rows close together in time.
    //   round 2's dealing: the three orientations of one (bundle, decoder, level) as neighbours on ONE XCD - they read the SAME
    //     segment of the same rows while all planes shared one ray order (81 % of the row reads missed L2 without it); with an
    //     order per orientation they no longer share rays, and the dealing is 0-10 us slower than bundle-major.
    //   plane-major: every bundle of plane 0, then of plane 1, ...  12-14 us FASTER than bundle-major on room0's batches
    //     (4096 x 64: 86 us) and 10-35 us slower on freiburg1_desk's and scene0000's, with identical FETCH / atomic counters.
    // Measured (profiles/r03/n_*): with the same pixels through lenses of different focal length, bundle-major costs
    // 110 / 97 / 83 / 81 / 80 us at a horizontal field of view of 118 / 90 / 67 / 53 / 37 degrees where plane-major stays at
    // 99 / 87 / 87 / 88 / 90 - the orders cross near 80 degrees.  The fan's extent in each plane comes from the ray ordering
    // kernel, through device memory (no host round trip); the SECOND largest of the three is the criterion (the largest is
    // ~360 degrees in the plane the camera looks down on).
    bool plane_major = false;
    if (RENDER && perm) {
        const float* fan = (const float*)(perm + (size_t)ESLAM_RAY_ORDERS * R);
        const float f0 = fan[0], f1 = fan[1], f2 = fan[2];
        const float second = fmaxf(fminf(f0, f1), fminf(fmaxf(f0, f1), f2));
        plane_major = second >= 1.4f;
    }
    int bidx, pi;
    if (plane_major) { bidx = bid % nbundles; pi = bid / nbundles; }
    else { pi = bid % NPLW; bidx = bid / NPLW; }
    if (bidx >= nbundles || pi >= NPLW) return;
    int npass = 1;
    if constexpr (PAIR) {
        const int item = (int)shoff.o[pi] & 0xFF;
        pi = item & 15;
        npass = item >> 4;
    }
    const int d = pi / 6, o = (pi % 6) >> 1, lvl = pi & 1;
    const eslam_plane_t& P = planes.p[pi];
    // GZ: thread (j, c) fetches W1[j][lvl * 32 + c] of the plane's decoder now and stores it behind the cell phase's own loads
    float gz_wv = 0.0f;
    if (GZ) gz_wv = (d ? gz_w1_rgb : gz_w1_sdf)[(threadIdx.x >> 5) * ESLAM_FEAT + lvl * ESLAM_C_DIM + (threadIdx.x & 31)];
    static_assert(!GZ || NT == ESLAM_HIDDEN * ESLAM_C_DIM, "one element of the slice per thread");
    const int pw = P.w, ph = P.h;
    const int psy = (int)P.stride_y, psx = (int)P.stride_x, psc = (int)P.stride_c;
    float* __restrict__ grad = P.grad;
    const int64_t npts = RENDER ? (int64_t)R * S : (int64_t)R;       // decode mode: R = N points, unit = 64 points
    const int nunits = RENDER ? R : (int)((npts + 63) / 64);
    const int per = RENDER ? S : 64;                                  // samples per unit
    const int u0 = bidx * bundle;
    const int nu = min(bundle, nunits - u0);
    const int n = nu * per;                                           // <= BM by construction of `bundle`

    bool swap = false;
    if (threadIdx.x == 0) { sbox[0] = 0x7FFFFFFF; sbox[1] = -1; sbox[2] = 0x7FFFFFFF; sbox[3] = -1; }
    __syncthreads();

    // (1) bilinear cell of every sample of the bundle (4 per thread), and the bundle's bounding box in the plane
    AxisCoord cax[SPT], cay[SPT];
    int cpt[SPT];
    int bx0 = 0x7FFFFFFF, bx1 = -1, by0 = 0x7FFFFFFF, by1 = -1;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int slot = threadIdx.x + k * NT;
        cpt[k] = -1;
        if (slot < n) {
            const int ui = u0 + slot / per, s = slot % per;
            const int unit = (RENDER && perm) ? perm[(size_t)o * R + ui] : ui;      // the order made for this plane's orientation
            const int64_t pt = RENDER ? (int64_t)unit * S + s : (int64_t)unit * 64 + s;
            if (pt < npts) {
                float x, y, z;
                if (RENDER) {
                    const float zz = z_vals[pt];
                    x = rays_o[unit * 3 + 0] + rays_d[unit * 3 + 0] * zz;
                    y = rays_o[unit * 3 + 1] + rays_d[unit * 3 + 1] * zz;
                    z = rays_o[unit * 3 + 2] + rays_d[unit * 3 + 2] * zz;
                } else {
                    x = z_vals[pt * 3 + 0]; y = z_vals[pt * 3 + 1]; z = z_vals[pt * 3 + 2];
                }
                x = norm_coord(x, bnd.lo[0], bnd.hi[0]);
                y = norm_coord(y, bnd.lo[1], bnd.hi[1]);
                z = norm_coord(z, bnd.lo[2], bnd.hi[2]);
                cax[k] = axis_coord((o == 2) ? y : x, pw);
                cay[k] = axis_coord((o == 0) ? y : z, ph);
                cpt[k] = (int)pt;
                bx0 = min(bx0, cax[k].i0); bx1 = max(bx1, cax[k].i0);
                by0 = min(by0, cay[k].i0); by1 = max(by1, cay[k].i0);
            }
        }
    }
    if (GZ) gz_w[(threadIdx.x & 31) * GZ_WP + (threadIdx.x >> 5)] = gz_wv;      // read in the walk, many barriers from here
    bx0 = wave_min_i(bx0); bx1 = wave_max_i(bx1);
    by0 = wave_min_i(by0); by1 = wave_max_i(by1);
    if (lane == 0) {
        atomicMin(&sbox[0], bx0); atomicMax(&sbox[1], bx1);
        atomicMin(&sbox[2], by0); atomicMax(&sbox[3], by1);
    }
    __syncthreads();
    // The sort key runs along the axis the bundle travels along ("minor" = fastest-varying), so that consecutive cells
    // of the sorted list are neighbours along it and share a texel column that is carried instead of flushed twice.
    const int bxmin = sbox[0], bxmax = sbox[1], bymin = sbox[2], bymax = sbox[3];
    __syncthreads();                                                  // sbox's memory is reused from here on
    if (bxmax < 0) return;                                            // no valid sample in this bundle
    swap = (bymax - bymin) > (bxmax - bxmin);                         // travels along y: column-major keys
    // Bundles whose cells fit a small box (the normal case: 32 neighbouring rays) are ordered by a counting sort over
    // the box - one LDS integer atomic per sample, one scan, one placement pass - instead of the 66-stage bitonic
    // network (50 us of this kernel's 165).  Rows of the box get one padding column so that "next cell along the minor
    // axis" never wraps into the next row.  Order inside a cell is arbitrary; the cell's sum does not depend on it
    // beyond float rounding.
    const int mmin = swap ? bymin : bxmin, mext = (swap ? bymax : bxmax) - mmin + 2;
    const int Mmin = swap ? bxmin : bymin, Mext = (swap ? bxmax : bymax) - Mmin + 1;
    const bool counting = (int64_t)mext * Mext <= 4 * BM;
    if (counting) {
        constexpr int WPT = 2 * BM / NT;                       // counter words per thread in the scan
        for (int i = threadIdx.x; i < 2 * BM; i += NT) cnt[i] = 0u;
        __syncthreads();
        unsigned loc[SPT], tick[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            loc[k] = 0; tick[k] = 0;
            if (cpt[k] >= 0) {
                const int im = swap ? cay[k].i0 : cax[k].i0, iM = swap ? cax[k].i0 : cay[k].i0;
                loc[k] = (unsigned)((iM - Mmin) * mext + (im - mmin));
                const unsigned sh = (loc[k] & 1u) * 16u;
                tick[k] = (atomicAdd(&cnt[loc[k] >> 1], 1u << sh) >> sh) & 0xFFFFu;
            }
        }
        __syncthreads();
        // exclusive scan of the counters: thread t owns words [WPT t, WPT t + WPT)
        unsigned w[WPT], local = 0;
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            w[j] = cnt[threadIdx.x * WPT + j];
            local += (w[j] & 0xFFFFu) + (w[j] >> 16);
        }
        const unsigned incl = wave_incl_sum_u(local);
        if (lane == WAVE - 1) swsum[wave] = incl;
        __syncthreads();
        unsigned run = incl - local, nvalid = 0;
        for (int wv = 0; wv < NT / WAVE; ++wv) {
            if (wv < wave) run += swsum[wv];
            nvalid += swsum[wv];
        }
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const unsigned lo16 = w[j] & 0xFFFFu, hi16 = w[j] >> 16;
            cnt[threadIdx.x * WPT + j] = run | ((run + lo16) << 16);
            run += lo16 + hi16;
        }
        __syncthreads();
        unsigned pos[SPT];
#pragma unroll
        for (int k = 0; k < SPT; ++k) pos[k] = ((cnt[loc[k] >> 1] >> ((loc[k] & 1u) * 16u)) & 0xFFFFu) + tick[k];
        __syncthreads();                                       // counters are dead: their memory becomes stm / stM
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
            if (cpt[k] >= 0) {
                const AxisCoord& am = swap ? cay[k] : cax[k];
                const AxisCoord& aM = swap ? cax[k] : cay[k];
                const unsigned q = pos[k];                  // records are stored in sorted order
                sxy[q] = ((unsigned)(cay[k].i0 * psy + cax[k].i0 * psx) << 2) | (unsigned)(am.i1 > am.i0) |
                         ((unsigned)(aM.i1 > aM.i0) << 1);
                sw[q] = (float4_t){(1.0f - am.t) * (1.0f - aM.t), (1.0f - am.t) * aM.t, am.t * (1.0f - aM.t), am.t * aM.t};
                sgrow[q] = cpt[k];
            }
        }
        for (int i = (int)nvalid + threadIdx.x; i < BM; i += NT) {
            sxy[i] = PAD_XY;
            sw[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
            sgrow[i] = 0;
        }
        __syncthreads();
    } else {
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int slot = threadIdx.x + k * NT;
        unsigned key = 0xFFFFFFFFu;
        if (cpt[k] >= 0) {
            const AxisCoord& am = swap ? cay[k] : cax[k];       // minor axis
            const AxisCoord& aM = swap ? cax[k] : cay[k];       // major axis
            const int cell = aM.i0 * (swap ? ph : pw) + am.i0;
            key = ((unsigned)cell << SLOT_BITS) | (unsigned)slot;
            txy[slot] = ((unsigned)(cay[k].i0 * psy + cax[k].i0 * psx) << 2) | (unsigned)(am.i1 > am.i0) |
                        ((unsigned)(aM.i1 > aM.i0) << 1);
            ttm[slot] = am.t;
            ttM[slot] = aM.t;
            trow[slot] = cpt[k];
        }
        skey[slot] = key;
    }
    __syncthreads();

    // (2) bitonic sort of the keys (invalid slots carry the maximum key and end up last).  Wave w owns elements
    // [256w, 256w+256): every compare-exchange distance j < 256 stays inside one wave's chunk and needs no workgroup
    // barrier (DS operations of a wave execute in order); only the stages with j >= 256 synchronise the workgroup.
    {
        const int wbase = wave * CH;
        for (int k = 2; k <= BM; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j >= CH) {
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < SPT / 2; ++t) {
                        const int p = threadIdx.x + t * NT;                       // pair index
                        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));      // lower element of the pair
                        const int l = i | j;
                        const unsigned a = skey[i], b2 = skey[l];
                        if ((a > b2) == ((i & k) == 0)) { skey[i] = b2; skey[l] = a; }
                    }
                    __syncthreads();
                } else {
#pragma unroll
                    for (int t = 0; t < SPT / 2; ++t) {
                        const int p = lane + t * WAVE;                            // pair index inside the wave's chunk
                        const int i = wbase + (((p & ~(j - 1)) << 1) | (p & (j - 1)));
                        const int l = i | j;
                        const unsigned a = skey[i], b2 = skey[l];
                        if ((a > b2) == ((i & k) == 0)) { skey[i] = b2; skey[l] = a; }
                    }
                    WAVE_SYNC();
                }
            }
        }
    }
    // records into sorted order, through registers (the temporaries and the final layout overlap)
    __syncthreads();
    unsigned pxy[SPT];
    float ptm[SPT], ptM[SPT];
    int prow[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const unsigned key = skey[threadIdx.x + k * NT];
        const bool valid = key != 0xFFFFFFFFu;
        const int slot = key & SLOT_MASK;
        pxy[k] = valid ? txy[slot] : PAD_XY;
        ptm[k] = valid ? ttm[slot] : 0.f;
        ptM[k] = valid ? ttM[slot] : 0.f;
        prow[k] = valid ? trow[slot] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int q = threadIdx.x + k * NT;
        const bool valid = pxy[k] != PAD_XY;
        sxy[q] = pxy[k];
        sw[q] = valid ? (float4_t){(1.0f - ptm[k]) * (1.0f - ptM[k]), (1.0f - ptm[k]) * ptM[k], ptm[k] * (1.0f - ptM[k]),
                                   ptm[k] * ptM[k]}
                      : (float4_t){0.f, 0.f, 0.f, 0.f};
        sgrow[q] = prow[k];
    }
    __syncthreads();
    }

    // (3) walk: wave w owns sorted entries [256w, 256w+256), 64 at a time.  Per 64-entry block every lane fetches ONE
    // entry's (xy, g_feat row) and the block's cell boundaries become two 64-bit scalar masks (ballots): "entry starts a
    // new cell" and "... which is the next cell along the minor axis and shares a texel column".  The serial part per
    // entry is then a scalar bit test, one LDS read of the lane's two weights and ONE packed FMA - the version that
    // carried (cell, tm, tM) in registers and rebuilt the weights per entry spent ~11 VALU instructions there and was
    // issue-bound.  The g_feat values of WALK_N entries are loaded ahead of the walk of the
    // previous WALK_N: a wave's loads, stores and atomics retire in order on one vmcnt counter, so a load issued BEHIND an
    // atomic would wait for it (~3000 cycles under load).
    const char* __restrict__ gcol = GZ ? (const char*)(g_feat + (size_t)d * (size_t)npts * 16)      // + row * 64 + j * 4 bytes
                                       : (const char*)(g_feat + d * 64 + lvl * 32);                 // + row * 512 + c * 4 bytes
    unsigned cur_xy = PAD_XY;                  // cell being accumulated (PAD_XY: none / padding, never flushed)
    unsigned last_xy = PAD_XY;                 // xy of the last entry of the previous block
    typedef typename std::conditional<DET, long long, float>::type acc_t;
    acc_t acc0 = 0, acc1 = 0;
    bool det_bad = false;                      // DET: a contribution of the current cell was not representable
    const int e0 = wave * CH;

    // Flush of a finished cell: lane (hx, c) adds its two sums (major-axis corners 0 and 1) for its minor-axis corner.
    // All addressing is 32-bit VALU arithmetic on a byte offset from the wave-uniform plane base (SGPR base + VGPR
    // offset form): a first version did 64-bit address arithmetic on the scalar unit, and with 32 waves per CU sharing
    // ONE scalar ALU the walk was SALU-bound (11 scalar instructions per entry).
    const unsigned lane_off = (unsigned)(c * psc) << 2;
    const unsigned dm_bytes = (unsigned)(swap ? psy : psx) << 2, dM_bytes = (unsigned)(swap ? psx : psy) << 2;
    char* __restrict__ gbytes = DET ? (char*)(shadow + shoff.o[pi]) : (char*)grad;
    float* const gz_as = gz_a + (GZ ? wave * WAVE : 0);
    if constexpr (GZ) {
        // The rank-16 walk: four consecutive sorted entries per step.  Lane (slot s = lane >> 4, j = lane & 15) takes entry
        // 4 t + s of step t: ONE 16-byte LDS read of the entry's four weights, ONE row load (the four slots fetch four 64-byte
        // rows with one instruction, the row number comes from LDS: no v_readlane), two packed FMAs into the four sums
        // k = 2 hx + row - and one scalar test of the step's four `fresh` bits.  A cell's sums are thus held as four partial
        // sums per (k, j), one per slot; the flush adds them.  tests/quad_walk_ref.py restates the bookkeeping in numpy.
        //   (One entry per step - 64 lanes (hx, row, j), every row load fetching 16 distinct floats into 64 lanes, v_readlane +
        //   load + LDS read + bit test + wait + FMA + branch per entry - was 4-5 us slower in the walk and, with its flush's two
        //   more LDS round trips, 12-13 us in all: DESIGN.md section 5 "Four entries per step".)
        // (the lane-derived addresses of the walk are formed HERE: derived from `lane` itself the compiler forms them at the kernel's
        // start and keeps them through the cell and sort phases, whose registers are the kernel's peak)
        // PAIR, two walks: the second decoder's element of the slice, fetched now (behind the sort, whose registers are the kernel's peak)
        // and stored between the passes
        // (its addresses come from an opaque copy of the thread number: shared with the first slice's, formed at the kernel's
        // start, they would be kept through the sort)
        float gz_wv2 = 0.0f;
        unsigned wt = threadIdx.x;
        if constexpr (PAIR) {
            asm volatile("" : "+v"(wt));
            if (npass > 1) gz_wv2 = gz_w1_rgb[(wt >> 5) * ESLAM_FEAT + lvl * ESLAM_C_DIM + (wt & 31)];
        }
        int wl = lane;
        // PAIR: the walk runs once per decoder over the same records.  The loop stays rolled: the walk's body is most of the
        // kernel's code and has to fit the instruction cache once.  (wl is made opaque INSIDE the loop: the lane-derived
        // addresses are formed anew in each pass, not kept as loop invariants)
#pragma nounroll
        for (int pass = 0; pass < (PAIR ? npass : 1); ++pass) {
        asm volatile("" : "+v"(wl));
        const int s = wl >> 4, whx = wl >> 5, wc = wl & 31;    // accumulating role (s, j); flushing role (hx, c)
        const unsigned wlane_off = (unsigned)(wc * psc) << 2;
        const int up1 = ((wl + WAVE - 1) & (WAVE - 1)) << 2;         // ds_bpermute address of the lane below
        if constexpr (PAIR) {
            gcol = (const char*)(g_feat + (size_t)(d + pass) * (size_t)npts * 16);
            gbytes = (char*)planes.p[pi + pass * (NPL / 2)].grad;
            cur_xy = PAD_XY;
            last_xy = PAD_XY;
        }
        float2_t alo = {0.f, 0.f}, ahi = {0.f, 0.f};             // k = 0, 1 (hx = 0: rows 0, 1) and k = 2, 3 (hx = 1)
        // Flush of a finished cell.  The slots' partial sums are added by a transposing exchange - lane bit 4, then lane bit 5 -
        // after which lane (s, j) holds the cell's sum for k = s: the layout gz_as[k * 16 + j] the expansion reads.  Then lane
        // (hx, c) forms sum_j W1[j][c] A[hx][row][j] for rows 0 and 1 - the cell's 64 sums through the wave's 256 bytes of LDS (a
        // half-wave reads ONE address: broadcast), the slice's row c from gz_w - and adds them with two atomics as the walk below.
        // The flush is what a wave WAITS for (every LDS round trip in it showed in the kernel's time), so it has as few as the
        // registers allow.
        auto flush4 = [&](const bool lower_half_only) {
            if (cur_xy == PAD_XY) return;
            // v_permlane16_swap: rows 1 and 3 (16 lanes each) of the first operand <-> rows 0 and 2 of the second; the sum of the
            // two results is k = (s & 1) over slots s and s ^ 1 (alo) and k = 2 + (s & 1) (ahi).  v_permlane32_swap: lanes 32-63 of
            // the first <-> lanes 0-31 of the second; the sum is k = s over all four slots.
            // (inline assembly with the two wait states a VALU-written operand needs inside the string: hipcc 7.x folds the sum
            // of the builtin's two results into twice the first one)
            float x0 = alo[0], y0 = alo[1], x1 = ahi[0], y1 = ahi[1];
            asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x0), "+v"(y0));
            asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x1), "+v"(y1));
            float r0 = x0 + y0, r1 = x1 + y1;
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(r0), "+v"(r1));
            gz_as[wl] = r0 + r1;
            WAVE_SYNC();
            const float4_t* const A = (const float4_t*)(gz_as + whx * 32);
            // (the slice's row is read anew in every flush: as a loop invariant the compiler keeps its 16 values in registers, so
            // the row's offset is made opaque to it)
            unsigned wrow = (unsigned)(wc * GZ_WP);
            asm volatile("" : "+v"(wrow));
            const float4_t* const Wc = (const float4_t*)(gz_w + wrow);
            float f0 = 0.0f, f1 = 0.0f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float4_t v0 = A[jj], v1 = A[4 + jj], wv = Wc[jj];
#pragma unroll
                for (int i = 0; i < 4; ++i) { f0 += wv[i] * v0[i]; f1 += wv[i] * v1[i]; }
                // summed where they stand: six reads at a time (24 registers; all twelve in flight would take 48; three at a
                // time were 3 us slower), three at a time in the 1024-sample kernel, whose eight waves per SIMD leave 64 registers
                if ((jj & 1) || SPT == 2) asm volatile("" : "+v"(f0), "+v"(f1));
            }
            WAVE_SYNC();                                  // (the next flush's write stays behind these reads)
            const unsigned o0 = (cur_xy & ~3u) + wlane_off + ((cur_xy & 1u) & (unsigned)whx) * dm_bytes;
            const unsigned o1 = o0 + ((cur_xy >> 1) & 1u) * dM_bytes;
            if (!lower_half_only || whx == 0) {
                atomicAdd((float*)(gbytes + o0), f0);
                atomicAdd((float*)(gbytes + o1), f1);
            }
        };
        struct Rec4 { unsigned xy; unsigned long long fresh, adjacent; };
        auto fetch4 = [&](int blk, unsigned prev_last) {
            Rec4 r;
            r.xy = sxy[e0 + blk * WAVE + wl];
            unsigned prev = (unsigned)__builtin_amdgcn_ds_bpermute(up1, (int)r.xy);
            if (wl == 0) prev = prev_last;
            const bool fresh = r.xy != prev;
            const bool adj = fresh && r.xy != PAD_XY && prev != PAD_XY && (prev & 1u) && (r.xy & ~3u) == (prev & ~3u) + dm_bytes;
            r.fresh = __ballot(fresh);
            r.adjacent = __ballot(adj);
            return r;
        };
        // A step with a `fresh` bit.  For every fresh entry kk, in order: the step's entries in front of it that are not yet
        // summed (slots < kk) still belong to the cell it closes; then the flush; then - next cell along the minor axis: its first
        // texel column is our second one - every lane keeps ITS OWN partial sums of that column (ahi -> alo: the slots are added
        // at the next flush anyway).  What is left in g - the slots from the last fresh entry on - is added by the step itself.
        auto close_cell = [&](const Rec4& rec, const int e, const int kk, const bool carry, const float4_t w4, float& g) {
            const float gk = (s < kk) ? g : 0.f;                // (selected, not multiplied: a padding entry's row is row 0)
            g = (s < kk) ? 0.f : g;
            alo += gk * w4.xy;
            ahi += gk * w4.zw;
            flush4(carry);
            alo = carry ? ahi : (float2_t){0.f, 0.f};
            ahi = (float2_t){0.f, 0.f};
            cur_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, e + kk);
        };
        // rows are requested WALK_Q steps (16 entries) ahead, two groups in flight: loads issued behind an atomic wait for it
        constexpr int WALK_Q = 4;
        const __amdgpu_buffer_rsrc_t grsrc4 = __builtin_amdgcn_make_buffer_rsrc((void*)gcol, 0, (int)((unsigned)npts * 64u), 0x00020000);
        const int j4 = (wl & 15) * 4;
        const int* const rlane = sgrow + s;                    // + the step's first entry
        const float4_t* const wlane4 = sw + s;
#define LOAD_Q(buf, eb, grp)                                                                  \
    _Pragma("unroll") for (int t = 0; t < WALK_Q; ++t) {                                      \
        const int row = rlane[(eb) + 4 * ((grp) * WALK_Q + t)];                               \
        buf[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grsrc4, (row << 6) + j4, 0, 0)); \
    }
#define WALK_Q4(buf, rec, grp, eb)                                                            \
    _Pragma("unroll") for (int t = 0; t < WALK_Q; ++t) {                                      \
        const int st = (grp) * WALK_Q + t;                                                    \
        const float4_t w4 = wlane4[(eb) + 4 * st];                                            \
        const unsigned nib = ((st < 8 ? fresh_lo : fresh_hi) >> (4 * (st & 7))) & 15u;        \
        float g = buf[t];                                                                     \
        for (unsigned m = nib; __builtin_expect(m != 0u, 0); m &= m - 1u) {                   \
            const int kk = __builtin_ctz(m);                                                  \
            close_cell(rec, 4 * st, kk, ((st < 8 ? adj_lo : adj_hi) >> (4 * (st & 7) + kk)) & 1u, w4, g); \
        }                                                                                     \
        alo += g * w4.xy;           /* padding entries have zero weights and belong to no cell */ \
        ahi += g * w4.zw;                                                                     \
    }
        constexpr int nblk = CH / WAVE;
        constexpr int ngrp = WAVE / (4 * WALK_Q);              // groups per 64-entry record block (even)
        float ga[WALK_Q], gb[WALK_Q];
        Rec4 rec = fetch4(0, PAD_XY);
        LOAD_Q(ga, e0, 0)
        if constexpr (PAIR) {
            // the second pass reads the colour decoder's slice: every wave has left the first pass's last flush before it is
            // replaced (the pass's first record block and row loads are already under way)
            if (pass == 1) {
                __syncthreads();
                asm volatile("" : "+v"(wt));
                gz_w[(wt & 31) * GZ_WP + (wt >> 5)] = gz_wv2;
                __syncthreads();
            }
        }
#pragma unroll 1
        for (int blk = 0; blk < nblk; ++blk) {
            if ((unsigned)__builtin_amdgcn_readfirstlane((int)rec.xy) == PAD_XY) break;   // sorted: everything from here is padding
            last_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, WAVE - 1);
            Rec4 nxt = rec;
            if (blk + 1 < nblk) nxt = fetch4(blk + 1, last_xy);
            const int ebase = e0 + blk * WAVE;
            const unsigned fresh_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.fresh);
            const unsigned fresh_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.fresh >> 32));
            const unsigned adj_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.adjacent);
            const unsigned adj_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.adjacent >> 32));
#pragma unroll
            for (int g2 = 0; g2 < ngrp; g2 += 2) {
                LOAD_Q(gb, ebase, g2 + 1)
                WALK_Q4(ga, rec, g2, ebase)
                if (g2 + 2 < ngrp) {
                    LOAD_Q(ga, ebase, g2 + 2)
                } else if (blk + 1 < nblk) {
                    LOAD_Q(ga, ebase + WAVE, 0)
                }
                WALK_Q4(gb, rec, g2 + 1, ebase)
            }
            rec = nxt;
        }
        flush4(false);
        }
#undef LOAD_Q
#undef WALK_Q4
        return;
    }
    // the walk of the full-width and fixed-point instantiations: one entry per step
    auto flush = [&](bool lower_half_only) {
        if (cur_xy != PAD_XY) {
            const acc_t f0 = acc0, f1 = acc1;
            const unsigned o0 = (cur_xy & ~3u) + lane_off + ((cur_xy & 1u) & (unsigned)hx) * dm_bytes;
            const unsigned o1 = o0 + ((cur_xy >> 1) & 1u) * dM_bytes;
            if (DET) {
                if (!lower_half_only || hx == 0) {           // the shadow mirrors the plane element for element: 8 bytes each
                    atomicAdd((unsigned long long*)(gbytes + 2 * (size_t)o0), (unsigned long long)f0);
                    atomicAdd((unsigned long long*)(gbytes + 2 * (size_t)o1), (unsigned long long)f1);
                    // a contribution that was NaN / Inf or beyond the fixed-point range (|g w| >= 2.6e5; __float2ll_rn would
                    // have saturated or wrapped it silently): poison the float gradient so that divergence stays visible
                    if (det_bad) {
                        atomicAdd((float*)((char*)grad + o0), __builtin_nanf(""));
                        atomicAdd((float*)((char*)grad + o1), __builtin_nanf(""));
                    }
                }
            } else if (!lower_half_only || hx == 0) {
                atomicAdd((float*)(gbytes + o0), (float)f0);
                atomicAdd((float*)(gbytes + o1), (float)f1);
            }
        }
    };

    struct Rec { unsigned xy; int row; unsigned long long fresh, adjacent; };     // row: BYTE offset of the g_feat row (row * 512)
    auto fetch = [&](int blk, unsigned prev_last) {
        Rec r;
        const int e = e0 + blk * WAVE + lane;
        r.xy = sxy[e];
        r.row = sgrow[e] * 512;
        unsigned prev = __shfl_up(r.xy, 1, WAVE);
        if (lane == 0) prev = prev_last;
        const bool fresh = r.xy != prev;
        const bool adj = fresh && r.xy != PAD_XY && prev != PAD_XY && (prev & 1u) && (r.xy & ~3u) == (prev & ~3u) + dm_bytes;
        r.fresh = __ballot(fresh);
        r.adjacent = __ballot(adj);
        return r;
    };
    constexpr int WALK_N = 8;      // entries per load-ahead group (2 groups in flight: 2*WALK_N VGPRs)
    const float2_t* const wlane = (const float2_t*)sw + hx;                    // + 2 * entry
    // A row load is TWO instructions: v_readlane of the row's byte offset into an SGPR, and a buffer load that adds that SGPR
    // (soffset) and the lane's channel offset (voffset) to the descriptor's base - the global_load form needed a VALU add
    // per entry in between, and the walk is bound by instruction issue.
    const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc((void*)gcol, 0, (int)((unsigned)npts * 512u - (unsigned)(d * 64 + lvl * 32) * 4u), 0x00020000);
    const int cvoff = c * 4;
#define LOAD_HALF(buf, rec, half)                                                             \
    _Pragma("unroll") for (int t = 0; t < WALK_N; ++t) {                                      \
        const int rowb = __builtin_amdgcn_readlane((rec).row, (half) * WALK_N + t);           \
        buf[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grsrc, cvoff, rowb, 0)); \
    }
#define WALK_HALF(buf, rec, half, ebase)                                                      \
    _Pragma("unroll") for (int t = 0; t < WALK_N; ++t) {                                      \
        const int idx = (half) * WALK_N + t;                                                  \
        const float2_t w2 = wlane[2 * ((ebase) + idx)];                                       \
        if (((idx < 32 ? fresh_lo : fresh_hi) >> (idx & 31)) & 1u) {     /* one s_bitcmp on a 32-bit scalar */ \
            if (((idx < 32 ? adj_lo : adj_hi) >> (idx & 31)) & 1u) {                          \
                /* next cell along the minor axis: its first texel column is our second one - keep those sums */ \
                flush(true);                                                                  \
                const acc_t s0 = __shfl_xor(acc0, 32, WAVE), s1 = __shfl_xor(acc1, 32, WAVE); \
                acc0 = hx ? (acc_t)0 : s0;                                                    \
                acc1 = hx ? (acc_t)0 : s1;                                                    \
                if (DET) {            /* det_bad travels with the carried column's sums and with nothing else */ \
                    const int carried_bad = __shfl_xor((int)det_bad, 32, WAVE);               \
                    det_bad = !hx && carried_bad;                                             \
                }                                                                             \
            } else {                                                                          \
                flush(false);                                                                 \
                det_bad = false;                                                              \
                acc0 = 0;                                                                     \
                acc1 = 0;                                                                     \
            }                                                                                 \
            cur_xy = (unsigned)__builtin_amdgcn_readlane((int)(rec).xy, idx);                 \
        }                                                                                     \
        const float g = buf[t];        /* padding entries have zero weights and belong to no cell */ \
        if (DET) {                                                                            \
            const float t0_ = g * w2[0], t1_ = g * w2[1];                                     \
            det_bad = det_bad || !(fabsf(t0_) < FIX_LIMIT) || !(fabsf(t1_) < FIX_LIMIT);      \
            acc0 += (acc_t)__float2ll_rn(t0_ * FIX_SCALE);                                    \
            acc1 += (acc_t)__float2ll_rn(t1_ * FIX_SCALE);                                    \
        } else {                                                                              \
            acc0 += (acc_t)(g * w2[0]);                                                       \
            acc1 += (acc_t)(g * w2[1]);                                                       \
        }                                                                                     \
    }

    const int nblk = CH / WAVE;
    const int ngrp = WAVE / WALK_N;                 // groups per 64-entry record block (even)
    float ga[WALK_N], gb[WALK_N];
    Rec rec = fetch(0, PAD_XY);
    LOAD_HALF(ga, rec, 0)
#pragma unroll 1
    for (int blk = 0; blk < nblk; ++blk) {
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)rec.xy) == PAD_XY) break;   // sorted: everything from here is padding
        last_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, WAVE - 1);
        Rec nxt = rec;
        if (blk + 1 < nblk) nxt = fetch(blk + 1, last_xy);
        const int ebase = e0 + blk * WAVE;
        const unsigned fresh_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.fresh);
        const unsigned fresh_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.fresh >> 32));
        const unsigned adj_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.adjacent);
        const unsigned adj_hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.adjacent >> 32));
#pragma unroll
        for (int g2 = 0; g2 < ngrp; g2 += 2) {
            LOAD_HALF(gb, rec, g2 + 1)
            WALK_HALF(ga, rec, g2, ebase)
            if (g2 + 2 < ngrp) {
                LOAD_HALF(ga, rec, g2 + 2)
            } else if (blk + 1 < nblk) {
                LOAD_HALF(ga, nxt, 0)
            }
            WALK_HALF(gb, rec, g2 + 1, ebase)
        }
        rec = nxt;
    }
#undef LOAD_HALF
#undef WALK_HALF
    flush(false);
}

// deterministic mode: float gradient += shadow * 2^-44, shadow cleared (it is all zero again for the next call)
__global__ __launch_bounds__(256) void scatter_fixed_to_float_kernel(float* __restrict__ grad, long long* __restrict__ shadow,
                                                                     int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const long long v = shadow[i];
        if (v != 0) {
            grad[i] += (float)((double)v * (1.0 / 17592186044416.0));
            shadow[i] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side (called from eslam_render_bwd.hip)
// ---------------------------------------------------------------------------------------------------------
int eslam_scatter_v2_init();

// perm [R] <- rays ordered by direction; chunks of SORT_MAX rays are ordered independently.  clear / clear_bytes: a buffer the
// same launch zeroes (NULL / 0: none).
static int ray_order_launch(const char* who, const float* rays_o, const float* rays_d, int R, int32_t* perm, void* clear,
                            int64_t clear_bytes, eslam_stream_t stream) {
    if (ray_order_check_args(who, rays_o, rays_d, R, perm, clear, clear_bytes)) return 1;
    if (R <= 0 && clear_bytes == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = eslam_scatter_v2_init()) return rc;
    const int key_bits = ray_order_key_bits(R);
    const int n_clear = ray_clear_blocks(clear_bytes);
    const int n_order = ray_order_blocks(R);
    hipLaunchKernelGGL(ray_order_kernel, dim3(n_order + n_clear), dim3(1024), ray_order_lds_bytes(key_bits), st,
                       rays_o, rays_d, R, perm, key_bits, n_order, (float*)clear, (long long)(clear_bytes >> 2));
    return eslam_check_launch("ray_order_kernel");
}

extern "C" int eslam_ray_order(const float* rays_o, const float* rays_d, int R, int32_t* perm, eslam_stream_t stream) {
    if (R <= 0) return 0;
    return ray_order_launch("eslam_ray_order", rays_o, rays_d, R, perm, nullptr, 0, stream);
}

extern "C" int eslam_ray_order_clear(const float* rays_o, const float* rays_d, int R, int32_t* perm, void* clear_ptr,
                                     int64_t clear_bytes, eslam_stream_t stream) {
    return ray_order_launch("eslam_ray_order_clear", rays_o, rays_d, R, perm, clear_ptr, clear_bytes, stream);
}

// perm: ray order to bundle by (render mode), or NULL for the given order
// Samples per workgroup (*bm_out).  2048 (512 threads x 4) halve the cell flushes of 1024; a batch whose 2048-sample bundles
// make fewer than SC_SMALL_WGS workgroups (most CUs would idle while a few walk 256 entries per wave) is cut into
// 1024-sample bundles walked by the same 512 threads (2 samples per thread, 128 sorted entries per wave): twice the
// workgroups, half the walk.  Measured (profiles/r03/c_*): 200 x 32 (84 workgroups) 50.9 -> 30.6 us; 1024 x 64 (384) 47.2 ->
// 50.6, 1024 x 96 (588) 55.1 -> 68.5, 2048 x 64 75.5 -> 89.7: from a few hundred workgroups on the kernel is throughput-bound
// and the extra cell flushes of the smaller bundles cost more than the shorter walk gains.
#define SC_SMALL_WGS 192
static int scatter_bundle_size(int per, int nunits, int* bm_out) {
    int bm = 2048;                                     // (the fixed-point kernel is instantiated for 2048 only)
    if (!eslam_deterministic()) {
        const int big = 2048 / per;
        const int nb = big > 0 ? (nunits + big - 1) / big : nunits;
        bm = (nb * NPL <= SC_SMALL_WGS && 1024 / per >= 1) ? 1024 : 2048;
    }
    *bm_out = bm;
    return bm / per;
}

// Samples per workgroup (1024 or 2048) the scatter of such a batch is launched with: render mode n = rays of S samples each,
// decode mode (S ignored) n = points.  Host arithmetic only; tests use it to see which instantiation a size exercises.
extern "C" int eslam_scatter_bundle_samples(int64_t n, int S, int render) {
    if (n <= 0 || (render && (S <= 0 || S > 256))) return 0;
    int bm = 0;
    (void)scatter_bundle_size(render ? S : 64, render ? (int)n : (int)((n + 63) / 64), &bm);
    return bm;
}

// whether the scatter launch of this mode can also run the decoder-gradient slab reduction (the production render path);
// the stand-alone dec_grad_reduce_kernel covers the rest
bool eslam_scatter_can_reduce(bool render) {
    return render && !eslam_deterministic();
}

// The paired grid of the rank-16 path (scatter_sort_kernel<PAIR>): where the SDF decoder's plane and the colour decoder's of
// one (orientation, level) agree in shape, one workgroup per bundle sorts once and walks twice.  Fewer workgroups, some of them
// longer: below SC_PAIR_WGS_PER_CU workgroups per CU the kernel is latency-bound and wants more workgroups, not fewer.
#define SC_PAIR_WGS_PER_CU 3
static int g_scatter_pairing = 1;                     // 0 never, 1 auto, 2 whenever a pair of planes allows it
static int g_last_scatter_paired = 0;

extern "C" int eslam_scatter_pairing(int mode) {
    const int prev = g_scatter_pairing;
    if (mode >= 0 && mode <= 2) g_scatter_pairing = mode;
    return prev;
}

extern "C" int eslam_last_scatter_paired(void) { return g_last_scatter_paired; }

// the auto rule: whether a render batch of n rays x S samples, npairs of whose six plane pairs agree, is paired on a device of
// `cus` compute units
extern "C" int eslam_scatter_pairs_auto(int64_t n, int S, int cus, int npairs) {
    if (n <= 0 || S <= 0 || S > 256 || cus <= 0 || npairs <= 0 || npairs > NPL / 2) return 0;
    int bm = 0;
    const int bundle = scatter_bundle_size(S, (int)n, &bm);
    const int64_t nbundles = (n + bundle - 1) / bundle;
    return nbundles * (NPL - npairs) >= (int64_t)SC_PAIR_WGS_PER_CU * cus;
}

// The work list of a bundle (PAIR in the kernel's header comment) into so.o: the planes that stay single in plane order, then
// the pairs p, p + 6 that can share a workgroup - same cells, same offsets, both with a gradient.  Returns the number of pairs.
// The order is measured (4096 x 64, shipped shapes: three coarse pairs, six fine planes; scatter_sort_kernel in the replayed step,
// profiles/r10/list_orders.txt): pairs first 85 - 89 us against the 12-plane grid's 79 - 83, pairs last 70 - 72.  A plane-major grid
// then starts with the fine planes' long workgroups and ends with the short ones; the same order WITHOUT pairing (twelve
// single planes, fine ones first) gives 72 - 77.
static int scatter_work_list(const eslam_plane_t* planes, ShadowOff* so) {
    bool pair[NPL / 2];
    int n = 0, npairs = 0;
    for (int p = 0; p < NPL / 2; ++p) {
        const eslam_plane_t &a = planes[p], &b = planes[p + NPL / 2];
        pair[p] = a.w == b.w && a.h == b.h && a.stride_x == b.stride_x && a.stride_y == b.stride_y &&
                  a.stride_c == b.stride_c && a.grad && b.grad;
        if (pair[p]) ++npairs;
    }
    for (int pi = 0; pi < NPL; ++pi)
        if (!pair[pi % (NPL / 2)]) so->o[n++] = pi | (1 << 4);
    for (int p = 0; p < NPL / 2; ++p)
        if (pair[p]) so->o[n++] = p | (2 << 4);
    so->o[0] |= (int64_t)n << 8;
    return npairs;
}

// compute units of the current device (0: unknown - the auto rule then does not pair)
static int scatter_device_cus() {
    constexpr int MAXDEV = 64;
    static int cus[MAXDEV];
    int devi = 0;
    if (hipGetDevice(&devi) != hipSuccess || devi < 0 || devi >= MAXDEV) return 0;
    if (cus[devi] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, devi) != hipSuccess || n <= 0) return 0;
        cus[devi] = n;
    }
    return cus[devi];
}

int eslam_scatter_v2(const eslam_plane_t* planes, const Bound& bnd, const float* rays_o, const float* rays_d,
                     const float* z_or_pts, int64_t R, int S, bool render, const float* g_feat, const int* perm,
                     hipStream_t st, const DecReduceArgs* red, const eslam_decoders_t* gz_dec) {
    PlaneSet ps;
    for (int i = 0; i < NPL; ++i) {
        ps.p[i] = planes[i];

    }
    const int64_t N = render ? R * S : R;
    const int nunits = render ? (int)R : (int)((N + 63) / 64);
    // the walk addresses g_feat rows and plane texels with 32-bit byte offsets from a uniform base (rank-16 path: 64-byte
    // rows from the decoder's half of gz[2][N][16], descriptor range N * 64 - inside the same limit, which the workspace's
    // layout and the decoder backward's stores keep)
    if (gz_dec && (!render || eslam_deterministic())) {
        eslam_set_error("scatter: the rank-16 path serves the float render mode only");
        return 1;
    }
    // gz[2][N][16]: the decoder backward's descriptor spans 2 N * 64 bytes, the walk's row offset goes up to N * 64 as an int
    static_assert(2 * 64 <= 512 && ESLAM_HIDDEN * 4 == 64, "the rank-16 rows' offsets lie inside the N * 512 limit checked below");
    if (gz_dec && (N * 128 >= ((int64_t)1 << 32) - 256 || N * 64 > INT32_MAX)) {
        eslam_set_error("scatter: %lld points exceed the 32-bit offset range of the 16-wide gradient rows", (long long)N);
        return 1;
    }
    if (N * 512 >= ((int64_t)1 << 32)) {
        eslam_set_error("scatter: %lld points exceed the 32-bit offset range of the feature-gradient buffer (8.3 M): split "
                        "the batch", (long long)N);
        return 1;
    }
    for (int i = 0; i < NPL; ++i) {
        const int64_t extent = (ESLAM_C_DIM - 1) * planes[i].stride_c + (int64_t)(planes[i].h - 1) * planes[i].stride_y +
                               (int64_t)(planes[i].w - 1) * planes[i].stride_x + 1;
        if (extent >= ((int64_t)1 << 30)) {
            eslam_set_error("scatter: plane %d spans %lld elements, limit 2^30", i, (long long)extent);
            return 1;
        }
    }
    const int per = render ? S : 64;
    // 2048 samples per workgroup (512 threads) halve the number of cell flushes of 1024; S up to 256 -> >= 8 rays
    int bm;
    const int bundle = scatter_bundle_size(per, nunits, &bm);
    for (int i = 0; i < NPL; ++i)
        if ((int64_t)planes[i].w * planes[i].h >= ((1 << 21) - 2)) {
            eslam_set_error("scatter: plane %d has %d x %d cells, limit 2^21", i, planes[i].h, planes[i].w);
            return 1;
        }
    const int nbundles = (nunits + bundle - 1) / bundle;
    // pairing is decided after the bundle size (scatter_sort_kernel<PAIR>; the rule: SC_PAIR_WGS_PER_CU)
    ShadowOff work = {};
    int npairs = 0;
    if (gz_dec && g_scatter_pairing != 0) npairs = scatter_work_list(planes, &work);
    const bool paired = npairs > 0 && (g_scatter_pairing == 2 || (int64_t)nbundles * (NPL - npairs) >=
                                                                     (int64_t)SC_PAIR_WGS_PER_CU * scatter_device_cus());
    g_last_scatter_paired = paired ? 1 : 0;
    dim3 grid(nbundles * (paired ? NPL - npairs : NPL));
    DecReduceArgs red_args = {};
    int red_blocks = 0;
    if (red) {
        if (!eslam_scatter_can_reduce(render)) {
            eslam_set_error("scatter: cannot carry the decoder-gradient reduction in this mode");
            return 1;
        }
        red_args = *red;
        red_blocks = (2 * DEC_RED_COLBLOCKS + 7) / 8 * 8;
        grid.x += red_blocks;
    }
#define LAUNCH_SC(RD, PERM, SS, ...)                                                                                      \
    hipLaunchKernelGGL((scatter_sort_kernel<RD, false, ##__VA_ARGS__>), grid, dim3(SC_NT), 0, st, ps, bnd, rays_o, rays_d, z_or_pts, \
                       PERM, (int)R, SS, g_feat, bundle, nbundles, (long long*)nullptr, work, red_args, red_blocks, \
                       gz_dec ? gz_dec->w1 : nullptr, gz_dec ? gz_dec->cw1 : nullptr)
    if (eslam_deterministic()) {
        // fixed-point scatter into the int64 shadow, then shadow -> float gradients (DET in the kernel's header comment)
        ShadowOff so;
        int64_t total = 0;
        for (int i = 0; i < NPL; ++i) {
            const int64_t numel = (int64_t)ESLAM_C_DIM * planes[i].h * planes[i].w;
            const int64_t extent = (ESLAM_C_DIM - 1) * planes[i].stride_c + (int64_t)(planes[i].h - 1) * planes[i].stride_y +
                                   (int64_t)(planes[i].w - 1) * planes[i].stride_x + 1;
            if (extent != numel) {
                eslam_set_error("scatter (deterministic mode): plane %d is not dense", i);
                return 1;
            }
            so.o[i] = total;
            total += numel;
        }
        // One shadow per DEVICE (the pointer is a device allocation of the device that is current now).  A shadow that has
        // been handed to a launch is never freed: a hipGraph captured earlier may still hold its address, so a larger scene
        // gets a new allocation and the old one stays (a few scenes per process at most).
        constexpr int MAXDEV = 64;
        static long long* shadows[MAXDEV];
        static int64_t shadow_ns[MAXDEV];
        static std::mutex shadow_mu;
        int devi = 0;
        if (hipGetDevice(&devi) != hipSuccess || devi < 0 || devi >= MAXDEV) {
            eslam_set_error("scatter (deterministic mode): no usable current device");
            return 2;
        }
        long long* shadow;
        {
            std::lock_guard<std::mutex> lk(shadow_mu);
            if (shadow_ns[devi] < total) {       // first use (an eager warm-up call; hipMalloc cannot be captured into a graph)
                hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
                (void)hipStreamIsCapturing(st, &cs);
                if (cs != hipStreamCaptureStatusNone) {
                    eslam_set_error("scatter (deterministic mode): run one eager iteration before capturing a graph");
                    return 1;
                }
                long long* fresh = nullptr;
                if (hipMalloc(&fresh, (size_t)total * 8) != hipSuccess || hipMemset(fresh, 0, (size_t)total * 8) != hipSuccess) {
                    eslam_set_error("scatter (deterministic mode): cannot allocate the %lld-element shadow", (long long)total);
                    return 2;
                }
                shadows[devi] = fresh;           // (the previous, smaller one is deliberately kept alive: see above)
                shadow_ns[devi] = total;
            }
            shadow = shadows[devi];
        }
        if (render)
            hipLaunchKernelGGL((scatter_sort_kernel<true, true>), grid, dim3(SC_NT), 0, st, ps, bnd, rays_o, rays_d,
                               z_or_pts, perm, (int)R, S, g_feat, bundle, nbundles, shadow, so, DecReduceArgs{}, 0, nullptr, nullptr);
        else
            hipLaunchKernelGGL((scatter_sort_kernel<false, true>), grid, dim3(SC_NT), 0, st, ps, bnd, rays_o, rays_d,
                               z_or_pts, (const int*)nullptr, (int)R, 64, g_feat, bundle, nbundles, shadow, so,
                               DecReduceArgs{}, 0, nullptr, nullptr);
        if (int rc = eslam_check_launch("scatter_sort_kernel<det>")) return rc;
        for (int i = 0; i < NPL; ++i) {
            const int64_t numel = (int64_t)ESLAM_C_DIM * planes[i].h * planes[i].w;
            hipLaunchKernelGGL(scatter_fixed_to_float_kernel, dim3((unsigned)((numel + 255) / 256 < 2048 ? (numel + 255) / 256 : 2048)),
                               dim3(256), 0, st, planes[i].grad, shadow + so.o[i], numel);
        }
        return eslam_check_launch("scatter_fixed_to_float_kernel");
    }
    if (gz_dec && paired) {
        if (bm == 1024) LAUNCH_SC(true, perm, S, 2, true, true);
        else LAUNCH_SC(true, perm, S, 4, true, true);
    } else if (gz_dec) {
        if (bm == 1024) LAUNCH_SC(true, perm, S, 2, true);
        else LAUNCH_SC(true, perm, S, 4, true);
    } else if (render) {
        if (bm == 1024) LAUNCH_SC(true, perm, S, 2);
        else LAUNCH_SC(true, perm, S);
    } else {
        if (bm == 1024) LAUNCH_SC(false, (const int*)nullptr, 64, 2);
        else LAUNCH_SC(false, (const int*)nullptr, 64);
    }
#undef LAUNCH_SC
    return eslam_check_launch("scatter_sort_kernel");
}

bool eslam_planes_channels_last(const eslam_plane_t* planes, int first, int count);
int eslam_validate_planes(const eslam_plane_t* planes, int first, int count);

int eslam_scatter_v2_init() {
    static bool done = false;
    if (done) return 0;
    if (hipFuncSetAttribute((const void*)ray_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            ORD_CELLS * (int)sizeof(unsigned)) != hipSuccess) {
        eslam_set_error("scatter: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        return 2;
    }
    done = true;
    return 0;
}
