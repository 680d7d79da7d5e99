// The plane-gradient scatter's phases as device functions: the body of scatter_sort_kernel (eslam_scatter.hip), which calls them
// top to bottom - cells, sort, walk.  Every function is inlined into the kernel; the phases meet in LDS (ScatterLds) and in the
// few registers named in their signatures.  The kernel sits on its register ceilings (80 VGPRs at 6 waves/SIMD, 64 at 8): the
// sort is the peak, and whatever the walk derives from the lane number is formed behind it (the opaque copies below).
#pragma once
#include <type_traits>
#include "eslam_decode_tile.h"
#include "eslam_dec_reduce.h"

typedef float float2_t __attribute__((ext_vector_type(2)));

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
// GZ (the rank-16 path, see mlp_bwd_kernel): g_feat holds gz[2][N][16], the gradient at the decoders' first hidden layer, and
//   the features' gradient W1^T . g_z1 is never formed per sample.  The walk sums w * g_z1 per cell in the 16-wide space - four
//   sorted entries per step, lane (slot = lane >> 4, j = lane & 15) with the entry's four corner sums, one 64-byte row per entry
//   shared by the six planes of a decoder - and the flush adds the slots and multiplies the cell's 2 x 2 x 16 sums by the plane's
//   [16, 32] slice of W1 (LDS, staged once per workgroup) before the same two atomics per lane (hx, c).  tests/rank16_ref.py
//   states what is computed, tests/quad_walk_ref.py restates the walk's bookkeeping in numpy.
constexpr int SC_NT = 512;
constexpr int GZ_WP = 20;                           // pitch (floats) of the W1 slice's rows [c][j]: 16-byte aligned, conflict-free
constexpr unsigned PAD_XY = 0xFFFFFFFFu;            // a record's xy word: padding behind the bundle's valid samples

// DET: where each plane's part of the int64 shadow starts (elements)
struct ShadowOff { int64_t o[NPL]; };
// PAIR: what the grid runs over per bundle instead of the 12 planes - entry w is plane[w], walked walks[w] times (2: also
// plane[w] + 6, the colour decoder's plane of the same orientation and level); n entries.  scatter_work_list fills it.
// (ints: the kernel reads its entry with one scalar load; a byte of the argument block takes a vector load and a readfirstlane)
struct ScatterWork {
    int plane[NPL];
    int walks[NPL];
    int n;
};
// The kernel's one argument.  An instantiation reads only the fields of its mode (behind the `:`).
struct ScatterArgs {
    PlaneSet planes;
    Bound bnd;
    const float* rays_o;          // RENDER
    const float* rays_d;          // RENDER
    const float* z_or_pts;        // RENDER ? z_vals [R, S] : points [N, 3]
    const int* perm;              // RENDER: the ray orders and the fan extents behind them, or NULL for the given order
    int R, S;                     // RENDER ? R rays of S samples : R points (S unused)
    const float* g_feat;          // GZ ? gz [2][N][16] : the features' gradient [N][128]
    int bundle, nbundles;         // units (rays; 64 points) per workgroup, workgroups per plane
    long long* shadow;            // DET
    ShadowOff shoff;              // DET
    ScatterWork work;             // PAIR
    DecReduceArgs red;            // RENDER && !DET, red_blocks > 0
    int red_blocks;               // RENDER && !DET
    const float* gz_w1_sdf;       // GZ: the decoders' first-layer weights [16][64]
    const float* gz_w1_rgb;       // GZ
};

template <bool RENDER> __device__ __forceinline__ int64_t scatter_npts(const ScatterArgs& a) {
    return RENDER ? (int64_t)a.R * a.S : (int64_t)a.R;            // decode mode: R = N points
}

// ---------------------------------------------------------------------------------------------------------
// LDS
// ---------------------------------------------------------------------------------------------------------
// 6*BM words (48 KB at BM = 2048; 3 workgroups per CU), three views of them, in the order they live:
//   cells + counting sort   cnt   [0, 2 BM)          4 BM packed 16-bit counters
//                           swsum [2 BM, +64)        per-wave totals of the scan
//                           box   [2 BM + 64, +4)    bounding box of the bundle's cells; registers from the barrier behind
//                                                    scatter_bundle_box on
//                           cnt is dead at the barrier behind the placement's reads (pos[]); swsum before it
//   bitonic fallback        skey  [0, BM)            (cell << SLOT_BITS) | local sample slot
//                           txy   [BM, 2 BM)         slot-indexed temporaries of the records: xy word,
//                           ttm   [2 BM + 128, +BM)  minor-axis and
//                           ttM   [3 BM + 128, +BM)  major-axis fraction,
//                           trow  [4 BM + 128, +BM)  point index (behind box / swsum, to 5 BM + 128)
//                           all dead at the barrier behind their read into registers (scatter_sort_bitonic's last but one)
//   the walk's records, in SORTED order, written by either sort over whatever it used:
//                           sw    [0, 4 BM) float4   bilinear weights of the entry for lane halves hx = 0 / 1 and rows 0 / 1:
//                                                    ((1-tm)(1-tM), (1-tm)tM, tm(1-tM), tm tM) - a lane reads its (row 0, row 1)
//                                                    pair with one ds_read_b64, so the per-entry VALU work of the walk is ONE
//                                                    packed FMA
//                           sxy   [4 BM, 5 BM)       byte offset of texel (x0,y0) << 2 | minor-axis step flag | major flag << 1;
//                                                    PAD_XY = padding
//                           sgrow [5 BM, 6 BM)       row of g_feat (global point index)
//                           live to the kernel's end (PAIR: through both walks)
// The reduction role uses the words as plain floats and never meets the others.
template <int SPT> struct ScatterLds {
    static constexpr int BM = SPT * SC_NT;
    static constexpr int WORDS = 6 * BM;
    unsigned* raw;
    __device__ __forceinline__ float4_t* sw() const { return (float4_t*)raw; }
    __device__ __forceinline__ unsigned* sxy() const { return raw + 4 * BM; }
    __device__ __forceinline__ int* sgrow() const { return (int*)(raw + 5 * BM); }
    __device__ __forceinline__ unsigned* cnt() const { return raw; }
    __device__ __forceinline__ unsigned* swsum() const { return raw + 2 * BM; }
    __device__ __forceinline__ int* box() const { return (int*)(raw + 2 * BM + 64); }
    __device__ __forceinline__ unsigned* skey() const { return raw; }
    __device__ __forceinline__ unsigned* txy() const { return raw + BM; }
    __device__ __forceinline__ float* ttm() const { return (float*)(raw + 2 * BM + 128); }
    __device__ __forceinline__ float* ttM() const { return (float*)(raw + 3 * BM + 128); }
    __device__ __forceinline__ int* trow() const { return (int*)(raw + 4 * BM + 128); }
};

// ---------------------------------------------------------------------------------------------------------
// (1) cells
// ---------------------------------------------------------------------------------------------------------
// a thread's SPT samples: bilinear cell along the plane's two axes and point index (-1: no sample)
template <int SPT> struct ScatterCells {
    AxisCoord ax[SPT], ay[SPT];
    int pt[SPT];
};
struct ScatterBox { int xmin, xmax, ymin, ymax; };

// The bilinear cell of every sample of bundle `bidx` in a plane of orientation o and pw x ph texels (SPT per thread), and the
// box of this thread's cells.
template <bool RENDER, int SPT>
__device__ __forceinline__ void scatter_cells(const ScatterLds<SPT>& lds, const ScatterArgs& a, const int o, const int pw,
                                              const int ph, const int bidx, ScatterCells<SPT>& cl, ScatterBox& tb) {
    constexpr int NT = SC_NT;
    const float* __restrict__ rays_o = a.rays_o;
    const float* __restrict__ rays_d = a.rays_d;
    const float* __restrict__ z_vals = a.z_or_pts;
    const int* __restrict__ perm = a.perm;
    const int R = a.R, S = a.S;
    const int64_t npts = scatter_npts<RENDER>(a);                     // decode mode: R = N points, unit = 64 points
    const int nunits = RENDER ? R : (int)((npts + 63) / 64);
    const int per = RENDER ? S : 64;                                  // samples per unit
    const int u0 = bidx * a.bundle;
    const int nu = min(a.bundle, nunits - u0);
    const int n = nu * per;                                           // <= BM by construction of `bundle`

    int* const sbox = lds.box();
    if (threadIdx.x == 0) { sbox[0] = 0x7FFFFFFF; sbox[1] = -1; sbox[2] = 0x7FFFFFFF; sbox[3] = -1; }
    __syncthreads();

    int bx0 = 0x7FFFFFFF, bx1 = -1, by0 = 0x7FFFFFFF, by1 = -1;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int slot = threadIdx.x + k * NT;
        cl.pt[k] = -1;
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
                x = norm_coord(x, a.bnd.lo[0], a.bnd.hi[0]);
                y = norm_coord(y, a.bnd.lo[1], a.bnd.hi[1]);
                z = norm_coord(z, a.bnd.lo[2], a.bnd.hi[2]);
                cl.ax[k] = axis_coord((o == 2) ? y : x, pw);
                cl.ay[k] = axis_coord((o == 0) ? y : z, ph);
                cl.pt[k] = (int)pt;
                bx0 = min(bx0, cl.ax[k].i0); bx1 = max(bx1, cl.ax[k].i0);
                by0 = min(by0, cl.ay[k].i0); by1 = max(by1, cl.ay[k].i0);
            }
        }
    }
    tb = {bx0, bx1, by0, by1};
}

// The bundle's bounding box in the plane from the threads' boxes.  False: the bundle has no valid sample.  swap: the bundle
// travels along y.
template <int SPT>
__device__ __forceinline__ bool scatter_bundle_box(const ScatterLds<SPT>& lds, ScatterBox& b, bool& swap) {
    int* const sbox = lds.box();
    const int lane = threadIdx.x & 63;
    int bx0 = wave_min_i(b.xmin), bx1 = wave_max_i(b.xmax);
    int by0 = wave_min_i(b.ymin), by1 = wave_max_i(b.ymax);
    if (lane == 0) {
        atomicMin(&sbox[0], bx0); atomicMax(&sbox[1], bx1);
        atomicMin(&sbox[2], by0); atomicMax(&sbox[3], by1);
    }
    __syncthreads();
    // The sort key runs along the axis the bundle travels along ("minor" = fastest-varying), so that consecutive cells
    // of the sorted list are neighbours along it and share a texel column that is carried instead of flushed twice.
    b = {sbox[0], sbox[1], sbox[2], sbox[3]};
    __syncthreads();                                                  // sbox's memory is reused from here on
    if (b.xmax < 0) return false;                                     // no valid sample in this bundle
    swap = (b.ymax - b.ymin) > (b.xmax - b.xmin);                     // travels along y: column-major keys
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// (2) sort
// ---------------------------------------------------------------------------------------------------------
// A record's xy word (ScatterLds) from the sample's cell along x and y and the same two as (minor, major), and its four
// weights from the fractions along (minor, major): what both sorts write.
__device__ __forceinline__ unsigned scatter_record_xy(const AxisCoord& ax, const AxisCoord& ay, const AxisCoord& am,
                                                      const AxisCoord& aM, const int psy, const int psx) {
    return ((unsigned)(ay.i0 * psy + ax.i0 * psx) << 2) | (unsigned)(am.i1 > am.i0) | ((unsigned)(aM.i1 > aM.i0) << 1);
}
__device__ __forceinline__ float4_t scatter_record_weights(const float tm, const float tM) {
    return (float4_t){(1.0f - tm) * (1.0f - tM), (1.0f - tm) * tM, tm * (1.0f - tM), tm * tM};
}

// Counting sort over the bundle's box, whose minor axis starts at mmin and is mext wide (one padding column included) and whose
// major axis starts at Mmin: one LDS integer atomic per sample, one scan, one placement pass.
template <int SPT>
__device__ __forceinline__ void scatter_sort_counting(const ScatterLds<SPT>& lds, const ScatterCells<SPT>& cl, const bool swap,
                                                      const int mmin, const int mext, const int Mmin, const int psy,
                                                      const int psx) {
    constexpr int NT = SC_NT, BM = SPT * NT;
    constexpr int WPT = 2 * BM / NT;                       // counter words per thread in the scan
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* const cnt = lds.cnt();
    unsigned* const swsum = lds.swsum();
    float4_t* const sw = lds.sw();
    unsigned* const sxy = lds.sxy();
    int* const sgrow = lds.sgrow();
    for (int i = threadIdx.x; i < 2 * BM; i += NT) cnt[i] = 0u;
    __syncthreads();
    unsigned loc[SPT], tick[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        loc[k] = 0; tick[k] = 0;
        if (cl.pt[k] >= 0) {
            const int im = swap ? cl.ay[k].i0 : cl.ax[k].i0, iM = swap ? cl.ax[k].i0 : cl.ay[k].i0;
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
    __syncthreads();                                       // counters are dead: their memory becomes the records
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        if (cl.pt[k] >= 0) {
            const AxisCoord& am = swap ? cl.ay[k] : cl.ax[k];
            const AxisCoord& aM = swap ? cl.ax[k] : cl.ay[k];
            const unsigned q = pos[k];                  // records are stored in sorted order
            sxy[q] = scatter_record_xy(cl.ax[k], cl.ay[k], am, aM, psy, psx);
            sw[q] = scatter_record_weights(am.t, aM.t);
            sgrow[q] = cl.pt[k];
        }
    }
    for (int i = (int)nvalid + threadIdx.x; i < BM; i += NT) {
        sxy[i] = PAD_XY;
        sw[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
        sgrow[i] = 0;
    }
    __syncthreads();
}

// The fallback for boxes too large for the counters: a bitonic sort of (cell, slot) keys, the records through slot-indexed
// temporaries.  mlen: the plane's length along the minor axis.
template <int SPT>
__device__ __forceinline__ void scatter_sort_bitonic(const ScatterLds<SPT>& lds, const ScatterCells<SPT>& cl, const bool swap,
                                                     const int mlen, const int psy, const int psx) {
    constexpr int NT = SC_NT, BM = SPT * NT;
    constexpr int CH = WAVE * SPT;                     // the chunk of a wave
    constexpr int SLOT_BITS = (BM == 1024) ? 10 : 11;
    constexpr unsigned SLOT_MASK = BM - 1;
    static_assert(BM == 1024 || BM == 2048, "bundle size");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* const skey = lds.skey();
    unsigned* const txy = lds.txy();
    float* const ttm = lds.ttm();
    float* const ttM = lds.ttM();
    int* const trow = lds.trow();
    float4_t* const sw = lds.sw();
    unsigned* const sxy = lds.sxy();
    int* const sgrow = lds.sgrow();
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int slot = threadIdx.x + k * NT;
        unsigned key = 0xFFFFFFFFu;
        if (cl.pt[k] >= 0) {
            const AxisCoord& am = swap ? cl.ay[k] : cl.ax[k];       // minor axis
            const AxisCoord& aM = swap ? cl.ax[k] : cl.ay[k];       // major axis
            const int cell = aM.i0 * mlen + am.i0;
            key = ((unsigned)cell << SLOT_BITS) | (unsigned)slot;
            txy[slot] = scatter_record_xy(cl.ax[k], cl.ay[k], am, aM, psy, psx);
            ttm[slot] = am.t;
            ttM[slot] = aM.t;
            trow[slot] = cl.pt[k];
        }
        skey[slot] = key;
    }
    __syncthreads();

    // bitonic sort of the keys (invalid slots carry the maximum key and end up last).  Wave w owns elements
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
        sw[q] = valid ? scatter_record_weights(ptm[k], ptM[k]) : (float4_t){0.f, 0.f, 0.f, 0.f};
        sgrow[q] = prow[k];
    }
    __syncthreads();
}

// Sorts the bundle's samples by cell into the walk's records.
// Bundles whose cells fit a small box (the normal case: 32 neighbouring rays) are ordered by a counting sort over
// the box instead of the 66-stage bitonic network (50 us of this kernel's 165).  Rows of the box get one padding column so
// that "next cell along the minor axis" never wraps into the next row.  Order inside a cell is arbitrary; the cell's sum
// does not depend on it beyond float rounding.
template <int SPT>
__device__ __forceinline__ void scatter_sort(const ScatterLds<SPT>& lds, const ScatterCells<SPT>& cl, const ScatterBox& b,
                                             const bool swap, const int pw, const int ph, const int psy, const int psx) {
    constexpr int BM = SPT * SC_NT;
    const int mmin = swap ? b.ymin : b.xmin, mext = (swap ? b.ymax : b.xmax) - mmin + 2;
    const int Mmin = swap ? b.xmin : b.ymin, Mext = (swap ? b.xmax : b.ymax) - Mmin + 1;
    if ((int64_t)mext * Mext <= 4 * BM) scatter_sort_counting<SPT>(lds, cl, swap, mmin, mext, Mmin, psy, psx);
    else scatter_sort_bitonic<SPT>(lds, cl, swap, swap ? ph : pw, psy, psx);
}

// ---------------------------------------------------------------------------------------------------------
// (3) walk
// ---------------------------------------------------------------------------------------------------------
// Wave w owns sorted entries [CH w, CH w + CH), 64 at a time.  Per 64-entry block every lane fetches ONE entry's record and the
// block's cell boundaries become two 64-bit scalar masks (ballots): "entry starts a new cell" and "... which is the next cell
// along the minor axis and shares a texel column".  The serial part per entry is then a scalar bit test, one LDS read of the
// lane's weights and packed FMAs - the version that carried (cell, tm, tM) in registers and rebuilt the weights per entry spent
// ~11 VALU instructions there and was issue-bound.  The g_feat values of one group of entries are loaded
// ahead of the walk of the previous group: a wave's loads, stores and atomics retire in order on one vmcnt counter, so a load
// issued BEHIND an atomic would wait for it (~3000 cycles under load).
//
// A walk is a struct: what is uniform over the wave, the lane's roles, and the sums of the cell being accumulated.  It gives
// the driver below
//   N, GROUPS          values a lane holds per load group; groups per 64-entry block (even)
//   Rec fetch(blk, prev_last)           the lane's record of block blk and the block's two masks
//   load(buf, rec, ebase, grp)          requests group grp's g_feat values of the block whose first entry is ebase
//   walk(buf, rec, ebase, grp, masks)   accumulates them, flushing the cells that end
//   flush(lower_half_only)              adds the current cell's sums to the plane
struct WalkMasks { unsigned fresh_lo, fresh_hi, adj_lo, adj_hi; };

// The block loop of both walks: two load groups in flight, NBLK blocks of 64 entries from e0.  `primed` runs once the first
// block's record and first group are requested.  grp is a constant in every call once the group loop is unrolled.
template <int NBLK, class Walk, class Primed>
__device__ __forceinline__ void scatter_walk_blocks(Walk& w, const int e0, Primed&& primed) {
    constexpr int N = Walk::N, NGRP = Walk::GROUPS;
    unsigned last_xy = PAD_XY;                 // xy of the last entry of the previous block
    float ga[N], gb[N];
    typename Walk::Rec rec = w.fetch(0, PAD_XY);
    w.load(ga, rec, e0, 0);
    primed();
#pragma unroll 1
    for (int blk = 0; blk < NBLK; ++blk) {
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)rec.xy) == PAD_XY) break;   // sorted: everything from here is padding
        last_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, WAVE - 1);
        typename Walk::Rec nxt = rec;
        if (blk + 1 < NBLK) nxt = w.fetch(blk + 1, last_xy);
        const int ebase = e0 + blk * WAVE;
        const WalkMasks m = {(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.fresh),
                             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.fresh >> 32)),
                             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec.adjacent),
                             (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec.adjacent >> 32))};
#pragma unroll
        for (int g2 = 0; g2 < NGRP; g2 += 2) {
            w.load(gb, rec, ebase, g2 + 1);
            w.walk(ga, rec, ebase, g2, m);
            if (g2 + 2 < NGRP) {
                w.load(ga, rec, ebase, g2 + 2);
            } else if (blk + 1 < NBLK) {
                w.load(ga, nxt, ebase + WAVE, 0);
            }
            w.walk(gb, rec, ebase, g2 + 1, m);
        }
        rec = nxt;
    }
    w.flush(false);
}

// The walk of the full-width and fixed-point instantiations: one entry per step, lane = (x-corner hx, channel c) with the
// sums of the cell's rows y0, y1 in two registers.
template <bool DET, int SPT> struct ScatterWalkFull {
    typedef typename std::conditional<DET, long long, float>::type acc_t;
    static constexpr int N = 8;                  // WALK_N: entries per load-ahead group (2 groups in flight: 2*N VGPRs)
    static constexpr int GROUPS = WAVE / N;
    struct Rec { unsigned xy; int row; unsigned long long fresh, adjacent; };     // row: BYTE offset of the g_feat row (row * 512)

    const unsigned* sxy;
    const int* sgrow;
    const float2_t* wlane;                       // + 2 * entry
    __amdgpu_buffer_rsrc_t grsrc;
    char* __restrict__ gbytes;
    float* __restrict__ grad;
    int lane, hx, cvoff, e0;
    unsigned lane_off, dm_bytes, dM_bytes;
    unsigned cur_xy;                             // cell being accumulated (PAD_XY: none / padding, never flushed)
    acc_t acc0, acc1;
    bool det_bad;                                // DET: a contribution of the current cell was not representable

    // gcol: the plane's 32 columns of g_feat, gcol_bytes past the buffer's start; gbytes: what the sums are added to
    __device__ __forceinline__ ScatterWalkFull(const ScatterLds<SPT>& lds, const char* __restrict__ gcol, const unsigned gcol_bytes,
                                               const int64_t npts, char* __restrict__ gbytes_, float* __restrict__ grad_,
                                               const bool swap, const int psy, const int psx, const int psc)
        : sxy(lds.sxy()), sgrow(lds.sgrow()), gbytes(gbytes_), grad(grad_), cur_xy(PAD_XY), acc0(0), acc1(0), det_bad(false) {
        lane = threadIdx.x & 63;
        const int wave = threadIdx.x >> 6;
        hx = lane >> 5;                          // hx: corner along the MINOR axis
        const int c = lane & 31;
        e0 = wave * (WAVE * SPT);
        // Flush addressing is 32-bit VALU arithmetic on a byte offset from the wave-uniform plane base (SGPR base + VGPR
        // offset form): a first version did 64-bit address arithmetic on the scalar unit, and with 32 waves per CU sharing
        // ONE scalar ALU the walk was SALU-bound (11 scalar instructions per entry).
        lane_off = (unsigned)(c * psc) << 2;
        dm_bytes = (unsigned)(swap ? psy : psx) << 2;
        dM_bytes = (unsigned)(swap ? psx : psy) << 2;
        wlane = (const float2_t*)lds.sw() + hx;
        // A row load is TWO instructions: v_readlane of the row's byte offset into an SGPR, and a buffer load that adds that SGPR
        // (soffset) and the lane's channel offset (voffset) to the descriptor's base - the global_load form needed a VALU add
        // per entry in between, and the walk is bound by instruction issue.
        grsrc = __builtin_amdgcn_make_buffer_rsrc((void*)gcol, 0, (int)((unsigned)npts * 512u - gcol_bytes), 0x00020000);
        cvoff = c * 4;
    }

    // Flush of a finished cell: lane (hx, c) adds its two sums (major-axis corners 0 and 1) for its minor-axis corner.
    __device__ __forceinline__ void flush(const bool lower_half_only) {
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
    }

    __device__ __forceinline__ Rec fetch(const int blk, const unsigned prev_last) const {
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
    }

    __device__ __forceinline__ void load(float (&buf)[N], const Rec& rec, const int /*ebase*/, const int grp) const {
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const int rowb = __builtin_amdgcn_readlane(rec.row, grp * N + t);
            buf[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grsrc, cvoff, rowb, 0));
        }
    }

    __device__ __forceinline__ void walk(const float (&buf)[N], const Rec& rec, const int ebase, const int grp, const WalkMasks& m) {
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const int idx = grp * N + t;
            const float2_t w2 = wlane[2 * (ebase + idx)];
            if (((idx < 32 ? m.fresh_lo : m.fresh_hi) >> (idx & 31)) & 1u) {     // one s_bitcmp on a 32-bit scalar
                if (((idx < 32 ? m.adj_lo : m.adj_hi) >> (idx & 31)) & 1u) {
                    // next cell along the minor axis: its first texel column is our second one - keep those sums
                    flush(true);
                    const acc_t s0 = __shfl_xor(acc0, 32, WAVE), s1 = __shfl_xor(acc1, 32, WAVE);
                    acc0 = hx ? (acc_t)0 : s0;
                    acc1 = hx ? (acc_t)0 : s1;
                    if (DET) {            // det_bad travels with the carried column's sums and with nothing else
                        const int carried_bad = __shfl_xor((int)det_bad, 32, WAVE);
                        det_bad = !hx && carried_bad;
                    }
                } else {
                    flush(false);
                    det_bad = false;
                    acc0 = 0;
                    acc1 = 0;
                }
                cur_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, idx);
            }
            const float g = buf[t];        // padding entries have zero weights and belong to no cell
            if (DET) {
                const float t0_ = g * w2[0], t1_ = g * w2[1];
                det_bad = det_bad || !(fabsf(t0_) < FIX_LIMIT) || !(fabsf(t1_) < FIX_LIMIT);
                acc0 += (acc_t)__float2ll_rn(t0_ * FIX_SCALE);
                acc1 += (acc_t)__float2ll_rn(t1_ * FIX_SCALE);
            } else {
                acc0 += (acc_t)(g * w2[0]);
                acc1 += (acc_t)(g * w2[1]);
            }
        }
    }
};

// One pass of the rank-16 walk: four consecutive sorted entries per step.  Lane (slot s = lane >> 4, j = lane & 15) takes entry
// 4 t + s of step t: ONE 16-byte LDS read of the entry's four weights, ONE row load (the four slots fetch four 64-byte
// rows with one instruction, the row number comes from LDS: no v_readlane), two packed FMAs into the four sums
// k = 2 hx + row - and one scalar test of the step's four `fresh` bits.  A cell's sums are thus held as four partial
// sums per (k, j), one per slot; the flush adds them.  tests/quad_walk_ref.py restates the bookkeeping in numpy.
//   (One entry per step - 64 lanes (hx, row, j), every row load fetching 16 distinct floats into 64 lanes, v_readlane +
//   load + LDS read + bit test + wait + FMA + branch per entry - was 4-5 us slower in the walk and, with its flush's two
//   more LDS round trips, 12-13 us in all: DESIGN.md section 5 "Four entries per step".)
// wl is the caller's OPAQUE copy of the lane number: every lane-derived address of the walk is formed from it, in the
// constructor - derived from the lane number itself the compiler forms them at the kernel's start and keeps them through the
// cell and sort phases, whose registers are the kernel's peak.
template <int SPT> struct ScatterWalkRank16 {
    static constexpr int N = 4;                  // WALK_Q: rows are requested N steps (16 entries) ahead, two groups in flight:
                                                 // loads issued behind an atomic wait for it
    static constexpr int GROUPS = WAVE / (4 * N);
    struct Rec { unsigned xy; unsigned long long fresh, adjacent; };

    const unsigned* sxy;
    const int* rlane;                            // + the step's first entry
    const float4_t* wlane4;
    const float* gz_w;                           // the plane's slice of W1 [c][j], pitch GZ_WP
    float* gz_as;                                // the wave's 64 floats of exchange
    __amdgpu_buffer_rsrc_t grsrc4;
    char* __restrict__ gbytes;
    int wl, s, whx, wc, up1, j4, e0;             // accumulating role (s, j); flushing role (hx, c)
    unsigned wlane_off, dm_bytes, dM_bytes;
    unsigned cur_xy;                             // cell being accumulated (PAD_XY: none / padding, never flushed)
    float2_t alo, ahi;                           // k = 0, 1 (hx = 0: rows 0, 1) and k = 2, 3 (hx = 1)

    // gcol: the decoder's half of gz; gbytes: the plane the sums are added to
    __device__ __forceinline__ ScatterWalkRank16(const ScatterLds<SPT>& lds, const int wl_, const int wave, const float* gz_w_,
                                                 float* gz_a, const char* __restrict__ gcol, const int64_t npts,
                                                 char* __restrict__ gbytes_, const bool swap, const int psy, const int psx,
                                                 const int psc)
        : sxy(lds.sxy()), gz_w(gz_w_), gz_as(gz_a + wave * WAVE), gbytes(gbytes_), wl(wl_), cur_xy(PAD_XY) {
        s = wl >> 4; whx = wl >> 5; wc = wl & 31;
        e0 = wave * (WAVE * SPT);
        wlane_off = (unsigned)(wc * psc) << 2;
        dm_bytes = (unsigned)(swap ? psy : psx) << 2;
        dM_bytes = (unsigned)(swap ? psx : psy) << 2;
        up1 = ((wl + WAVE - 1) & (WAVE - 1)) << 2;         // ds_bpermute address of the lane below
        alo = (float2_t){0.f, 0.f};
        ahi = (float2_t){0.f, 0.f};
        grsrc4 = __builtin_amdgcn_make_buffer_rsrc((void*)gcol, 0, (int)((unsigned)npts * 64u), 0x00020000);
        j4 = (wl & 15) * 4;
        rlane = lds.sgrow() + s;
        wlane4 = lds.sw() + s;
    }

    // Flush of a finished cell.  The slots' partial sums are added by a transposing exchange - lane bit 4, then lane bit 5 -
    // after which lane (s, j) holds the cell's sum for k = s: the layout gz_as[k * 16 + j] the expansion reads.  Then lane
    // (hx, c) forms sum_j W1[j][c] A[hx][row][j] for rows 0 and 1 - the cell's 64 sums through the wave's 256 bytes of LDS (a
    // half-wave reads ONE address: broadcast), the slice's row c from gz_w - and adds them with two atomics as the full-width
    // walk does.  The flush is what a wave WAITS for (every LDS round trip in it showed in the kernel's time), so it has as few
    // as the registers allow.
    __device__ __forceinline__ void flush(const bool lower_half_only) {
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
    }

    __device__ __forceinline__ Rec fetch(const int blk, const unsigned prev_last) const {
        Rec r;
        r.xy = sxy[e0 + blk * WAVE + wl];
        unsigned prev = (unsigned)__builtin_amdgcn_ds_bpermute(up1, (int)r.xy);
        if (wl == 0) prev = prev_last;
        const bool fresh = r.xy != prev;
        const bool adj = fresh && r.xy != PAD_XY && prev != PAD_XY && (prev & 1u) && (r.xy & ~3u) == (prev & ~3u) + dm_bytes;
        r.fresh = __ballot(fresh);
        r.adjacent = __ballot(adj);
        return r;
    }

    // A step with a `fresh` bit.  For every fresh entry kk, in order: the step's entries in front of it that are not yet
    // summed (slots < kk) still belong to the cell it closes; then the flush; then - next cell along the minor axis: its first
    // texel column is our second one - every lane keeps ITS OWN partial sums of that column (ahi -> alo: the slots are added
    // at the next flush anyway).  What is left in g - the slots from the last fresh entry on - is added by the step itself.
    __device__ __forceinline__ void close_cell(const Rec& rec, const int e, const int kk, const bool carry, const float4_t w4,
                                               float& g) {
        const float gk = (s < kk) ? g : 0.f;                // (selected, not multiplied: a padding entry's row is row 0)
        g = (s < kk) ? 0.f : g;
        alo += gk * w4.xy;
        ahi += gk * w4.zw;
        flush(carry);
        alo = carry ? ahi : (float2_t){0.f, 0.f};
        ahi = (float2_t){0.f, 0.f};
        cur_xy = (unsigned)__builtin_amdgcn_readlane((int)rec.xy, e + kk);
    }

    __device__ __forceinline__ void load(float (&buf)[N], const Rec& /*rec*/, const int ebase, const int grp) const {
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const int row = rlane[ebase + 4 * (grp * N + t)];
            buf[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grsrc4, (row << 6) + j4, 0, 0));
        }
    }

    __device__ __forceinline__ void walk(const float (&buf)[N], const Rec& rec, const int ebase, const int grp, const WalkMasks& m) {
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const int st = grp * N + t;
            const float4_t w4 = wlane4[ebase + 4 * st];
            const unsigned nib = ((st < 8 ? m.fresh_lo : m.fresh_hi) >> (4 * (st & 7))) & 15u;
            float g = buf[t];
            for (unsigned mm = nib; __builtin_expect(mm != 0u, 0); mm &= mm - 1u) {
                const int kk = __builtin_ctz(mm);
                close_cell(rec, 4 * st, kk, ((st < 8 ? m.adj_lo : m.adj_hi) >> (4 * (st & 7) + kk)) & 1u, w4, g);
            }
            alo += g * w4.xy;           // padding entries have zero weights and belong to no cell
            ahi += g * w4.zw;
        }
    }
};
