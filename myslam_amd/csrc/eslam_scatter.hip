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
// What is built instead needs no LDS atomics on floats at all.  The rays arrive ordered by direction (eslam_ray_order_dev.h:
// neighbours in the order are rays through neighbouring pixels of one camera, which cross the same texels for most of their
// length), and
//
// scatter_sort_kernel one workgroup = one bundle of consecutive rays in that order x one plane (PAIR: x the two decoders' planes
//                     of one orientation and level where they agree in shape).  Its phases are eslam_scatter_dev.h:
//                     (1) cells    the bilinear cell of each of the bundle's <= 2048 samples and the cells' bounding box;
//                     (2) sort     the samples by cell, in LDS: a counting sort over the box, a bitonic network as the fallback
//                                  for boxes too large for the counters; either leaves the same sorted records;
//                     (3) walk     each wave takes a contiguous part of the sorted list; consecutive entries of one cell are
//                                  summed in registers and each cell is written once with two 256-B-shaped float atomics per
//                                  lane (x-corner, channel).  Two walks: one entry per step over the features' full-width
//                                  gradient (also the fixed-point one of the deterministic mode), and four entries per step
//                                  over the 16-wide hidden gradient (GZ, the rank-16 path), expanded by W1 once per cell.
//                                  PAIR walks the records twice, once per decoder.
//                     The first workgroups of the production launch are not scatter workgroups: they sum the decoder
//                     backward's gradient slabs (eslam_dec_reduce.h).
#include <mutex>
#include "eslam_scatter_dev.h"

// PAIR (rank-16 path): a workgroup may serve the two planes pi and pi + 6 of one (orientation, level) - the SDF decoder's and the
//   colour decoder's.  They bundle the same rays, and where they agree in resolution and strides (the host checks it pair by
//   pair: the reference's default colour planes are twice as fine at the fine level, so only the coarse pairs agree there) cells,
//   bounding box, sort and the sorted records are the same entry for entry: phases (1) and (2) run once and the walk runs twice
//   over the records that are still in LDS, per pass with the decoder's half of gz, its gradient plane and its slice of W1
//   (restaged between the passes: both slices do not fit beside the records at three workgroups per CU).  The grid runs over a
//   work list per bundle (ScatterWork) instead of the 12 planes: the planes left single in front (the fine planes: most cells,
//   most flushes, the longest workgroups), the agreeing pairs (two short walks over few cells) behind them, where they fill the
//   grid's tail.
template <bool RENDER, bool DET, int SPT = 4, bool GZ = false, bool PAIR = false>
__global__ __launch_bounds__(SC_NT) __attribute__((amdgpu_waves_per_eu(PAIR ? (SPT == 4 ? 6 : 8) : 2))) void scatter_sort_kernel(const ScatterArgs a) {
    constexpr int NT = SC_NT;
    static_assert(SPT == 2 || SPT == 4, "samples per thread");
    static_assert(!GZ || (RENDER && !DET), "GZ: the float render path only");
    static_assert(!PAIR || GZ, "PAIR: the rank-16 path only");
    static_assert(!GZ || NT == ESLAM_HIDDEN * ESLAM_C_DIM, "one element of the W1 slice per thread");
    __shared__ __attribute__((aligned(16))) unsigned lds_raw[ScatterLds<SPT>::WORDS];
    // GZ: + 2560 B for the plane's slice of W1 as [c][j] and + 2048 B of wave-private exchange (a cell's 64 sums): 53 760 B at
    // BM = 2048, three workgroups per CU as before
    __shared__ __attribute__((aligned(16))) float gz_w[GZ ? ESLAM_C_DIM * GZ_WP : 4];
    __shared__ __attribute__((aligned(16))) float gz_a[GZ ? NT : 4];
    const ScatterLds<SPT> lds = {lds_raw};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // The first red_blocks workgroups (a multiple of 8) are not scatter workgroups:
    // they sum the decoder-gradient slabs of the decoder backward that ran just before (eslam_dec_reduce.h), beside the
    // scatter's first workgroups instead of as a launch of their own in front of them.
    int red_blocks = 0;
    if constexpr (RENDER && !DET) {
        red_blocks = a.red_blocks;
        if (red_blocks > 0 && (int)blockIdx.x < red_blocks) {
            if ((int)blockIdx.x < 2 * DEC_RED_COLBLOCKS)
                dec_grad_reduce_block<NT>(a.red, blockIdx.x % DEC_RED_COLBLOCKS, blockIdx.x / DEC_RED_COLBLOCKS, (float*)lds_raw);
            return;
        }
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
    const int NPLW = PAIR ? a.work.n : NPL;            // planes (PAIR: entries of the work list) the grid runs over
    bool plane_major = false;
    if (RENDER && a.perm) {
        const float* fan = (const float*)(a.perm + (size_t)ESLAM_RAY_ORDERS * a.R);
        const float f0 = fan[0], f1 = fan[1], f2 = fan[2];
        const float second = fmaxf(fminf(f0, f1), fminf(fmaxf(f0, f1), f2));
        plane_major = second >= 1.4f;
    }
    int bidx, pi;
    if (plane_major) { bidx = bid % a.nbundles; pi = bid / a.nbundles; }
    else { pi = bid % NPLW; bidx = bid / NPLW; }
    if (bidx >= a.nbundles || pi >= NPLW) return;
    // PAIR: entry pi of the work list is a plane and the number of walks over its records
    int npass = 1;
    if constexpr (PAIR) {
        npass = a.work.walks[pi];
        pi = a.work.plane[pi];
    }
    const int d = pi / 6, o = (pi % 6) >> 1, lvl = pi & 1;
    const eslam_plane_t& P = a.planes.p[pi];
    const int pw = P.w, ph = P.h;
    const int psy = (int)P.stride_y, psx = (int)P.stride_x, psc = (int)P.stride_c;
    // GZ: thread (j, c) fetches W1[j][lvl * 32 + c] of the plane's decoder now and stores it behind the cell phase's own loads
    float gz_wv = 0.0f;
    if constexpr (GZ) gz_wv = (d ? a.gz_w1_rgb : a.gz_w1_sdf)[(threadIdx.x >> 5) * ESLAM_FEAT + lvl * ESLAM_C_DIM + (threadIdx.x & 31)];

    // (1) cells
    ScatterCells<SPT> cells;
    ScatterBox box;
    bool swap = false;
    scatter_cells<RENDER, SPT>(lds, a, o, pw, ph, bidx, cells, box);
    if constexpr (GZ) gz_w[(threadIdx.x & 31) * GZ_WP + (threadIdx.x >> 5)] = gz_wv;      // read in the walk, many barriers from here
    if (!scatter_bundle_box<SPT>(lds, box, swap)) return;

    // (2) sort: the kernel's register peak
    scatter_sort<SPT>(lds, cells, box, swap, pw, ph, psy, psx);

    // (3) walk
    const int64_t npts = scatter_npts<RENDER>(a);
    if constexpr (GZ) {
        // PAIR, two walks: the second decoder's element of the slice, fetched now (behind the sort, whose registers are the kernel's peak)
        // and stored between the passes
        // (its addresses come from an opaque copy of the thread number: shared with the first slice's, formed at the kernel's
        // start, they would be kept through the sort)
        float gz_wv2 = 0.0f;
        unsigned wt = threadIdx.x;
        if constexpr (PAIR) {
            asm volatile("" : "+v"(wt));
            if (npass > 1) gz_wv2 = a.gz_w1_rgb[(wt >> 5) * ESLAM_FEAT + lvl * ESLAM_C_DIM + (wt & 31)];
        }
        int wl = lane;
        // PAIR: the walk runs once per decoder over the same records.  The loop stays rolled: the walk's body is most of the
        // kernel's code and has to fit the instruction cache once.  (wl is made opaque INSIDE the loop: the lane-derived
        // addresses are formed anew in each pass, not kept as loop invariants)
#pragma nounroll
        for (int pass = 0; pass < (PAIR ? npass : 1); ++pass) {
            asm volatile("" : "+v"(wl));
            ScatterWalkRank16<SPT> walk(lds, wl, wave, gz_w, gz_a, (const char*)(a.g_feat + (size_t)(d + pass) * (size_t)npts * 16), npts,
                                        (char*)a.planes.p[pi + pass * (NPL / 2)].grad, swap, psy, psx, psc);
            scatter_walk_blocks<SPT>(walk, walk.e0, [&] {
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
            });
        }
    } else {
        // (DET is a template constant: the float instantiations hold no read of the shadow's fields)
        ScatterWalkFull<DET, SPT> walk(lds, (const char*)(a.g_feat + d * 64 + lvl * 32), (unsigned)(d * 64 + lvl * 32) * 4u, npts,
                                       DET ? (char*)(a.shadow + a.shoff.o[pi]) : (char*)P.grad, P.grad, swap, psy, psx, psc);
        scatter_walk_blocks<SPT>(walk, walk.e0, [] {});
    }
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

// The work list of a bundle (PAIR in the kernel's header comment): the planes that stay single in plane order, then
// the pairs p, p + 6 that can share a workgroup - same cells, same offsets, both with a gradient.  Returns the number of pairs.
// The order is measured (4096 x 64, shipped shapes: three coarse pairs, six fine planes; scatter_sort_kernel in the replayed step,
// profiles/r10/list_orders.txt): pairs first 85 - 89 us against the 12-plane grid's 79 - 83, pairs last 70 - 72.  A plane-major grid
// then starts with the fine planes' long workgroups and ends with the short ones; the same order WITHOUT pairing (twelve
// single planes, fine ones first) gives 72 - 77.
static int scatter_work_list(const eslam_plane_t* planes, ScatterWork* work) {
    bool pair[NPL / 2];
    int n = 0, npairs = 0;
    for (int p = 0; p < NPL / 2; ++p) {
        const eslam_plane_t &a = planes[p], &b = planes[p + NPL / 2];
        pair[p] = a.w == b.w && a.h == b.h && a.stride_x == b.stride_x && a.stride_y == b.stride_y &&
                  a.stride_c == b.stride_c && a.grad && b.grad;
        if (pair[p]) ++npairs;
    }
    for (int pi = 0; pi < NPL; ++pi)
        if (!pair[pi % (NPL / 2)]) { work->plane[n] = pi; work->walks[n++] = 1; }
    for (int p = 0; p < NPL / 2; ++p)
        if (pair[p]) { work->plane[n] = p; work->walks[n++] = 2; }
    work->n = n;
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

// elements from a plane's first to one past its last
static int64_t plane_extent(const eslam_plane_t& p) {
    return (ESLAM_C_DIM - 1) * p.stride_c + (int64_t)(p.h - 1) * p.stride_y + (int64_t)(p.w - 1) * p.stride_x + 1;
}

// What the kernel's 32-bit arithmetic can address, and what the mode can carry (1: refused, the message is set).
// The walk addresses g_feat rows and plane texels with 32-bit byte offsets from a uniform base (rank-16 path: 64-byte
// rows from the decoder's half of gz[2][N][16], descriptor range N * 64 - inside the same limit, which the workspace's
// layout and the decoder backward's stores keep).
static int scatter_check_limits(const eslam_plane_t* planes, int64_t N, bool render, bool gz, bool reduce) {
    if (gz && (!render || eslam_deterministic())) {
        eslam_set_error("scatter: the rank-16 path serves the float render mode only");
        return 1;
    }
    // gz[2][N][16]: the decoder backward's descriptor spans 2 N * 64 bytes, the walk's row offset goes up to N * 64 as an int
    static_assert(2 * 64 <= 512 && ESLAM_HIDDEN * 4 == 64, "the rank-16 rows' offsets lie inside the N * 512 limit checked below");
    if (gz && (N * 128 >= ((int64_t)1 << 32) - 256 || N * 64 > INT32_MAX)) {
        eslam_set_error("scatter: %lld points exceed the 32-bit offset range of the 16-wide gradient rows", (long long)N);
        return 1;
    }
    if (N * 512 >= ((int64_t)1 << 32)) {
        eslam_set_error("scatter: %lld points exceed the 32-bit offset range of the feature-gradient buffer (8.3 M): split "
                        "the batch", (long long)N);
        return 1;
    }
    for (int i = 0; i < NPL; ++i) {
        const int64_t extent = plane_extent(planes[i]);
        if (extent >= ((int64_t)1 << 30)) {
            eslam_set_error("scatter: plane %d spans %lld elements, limit 2^30", i, (long long)extent);
            return 1;
        }
    }
    for (int i = 0; i < NPL; ++i)
        if ((int64_t)planes[i].w * planes[i].h >= ((1 << 21) - 2)) {        // the bitonic fallback's keys: cell << 11 | slot
            eslam_set_error("scatter: plane %d has %d x %d cells, limit 2^21", i, planes[i].h, planes[i].w);
            return 1;
        }
    if (reduce && !eslam_scatter_can_reduce(render)) {
        eslam_set_error("scatter: cannot carry the decoder-gradient reduction in this mode");
        return 1;
    }
    return 0;
}

// How a batch of nunits units of `per` samples is launched.
struct ScatterPlan {
    int bm;                    // samples per workgroup: 1024 or 2048 (S up to 256 -> >= 8 rays of a 2048-sample bundle)
    int bundle, nbundles;      // units per workgroup, workgroups per plane
    bool paired;               // the grid runs over `work`, not over the 12 planes
    ScatterWork work;
    int red_blocks;            // reduction workgroups in front of the scatter's
    unsigned grid;
};

static ScatterPlan scatter_plan(const eslam_plane_t* planes, int per, int nunits, bool gz, bool reduce) {
    ScatterPlan p = {};
    p.bundle = scatter_bundle_size(per, nunits, &p.bm);
    p.nbundles = (nunits + p.bundle - 1) / p.bundle;
    // pairing is decided after the bundle size (scatter_sort_kernel<PAIR>; the rule: SC_PAIR_WGS_PER_CU)
    int npairs = 0;
    if (gz && g_scatter_pairing != 0) npairs = scatter_work_list(planes, &p.work);
    p.paired = npairs > 0 && (g_scatter_pairing == 2 || (int64_t)p.nbundles * (NPL - npairs) >=
                                                            (int64_t)SC_PAIR_WGS_PER_CU * scatter_device_cus());
    p.red_blocks = reduce ? (2 * DEC_RED_COLBLOCKS + 7) / 8 * 8 : 0;
    p.grid = (unsigned)(p.nbundles * (p.paired ? NPL - npairs : NPL) + p.red_blocks);
    return p;
}

// Deterministic mode: the int64 shadow of the current device, large enough for the planes, and each plane's offset in it.
// One shadow per DEVICE (the pointer is a device allocation of the device that is current now).  A shadow that has
// been handed to a launch is never freed: a hipGraph captured earlier may still hold its address, so a larger scene
// gets a new allocation and the old one stays (a few scenes per process at most).
static int scatter_shadow(const eslam_plane_t* planes, hipStream_t st, long long** shadow, ShadowOff* so) {
    int64_t total = 0;
    for (int i = 0; i < NPL; ++i) {
        const int64_t numel = (int64_t)ESLAM_C_DIM * planes[i].h * planes[i].w;
        if (plane_extent(planes[i]) != numel) {
            eslam_set_error("scatter (deterministic mode): plane %d is not dense", i);
            return 1;
        }
        so->o[i] = total;
        total += numel;
    }
    constexpr int MAXDEV = 64;
    static long long* shadows[MAXDEV];
    static int64_t shadow_ns[MAXDEV];
    static std::mutex shadow_mu;
    int devi = 0;
    if (hipGetDevice(&devi) != hipSuccess || devi < 0 || devi >= MAXDEV) {
        eslam_set_error("scatter (deterministic mode): no usable current device");
        return 2;
    }
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
    *shadow = shadows[devi];
    return 0;
}

template <bool RENDER, bool DET, int SPT, bool GZ, bool PAIR>
static void scatter_launch(const ScatterArgs& a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((scatter_sort_kernel<RENDER, DET, SPT, GZ, PAIR>), dim3(grid), dim3(SC_NT), 0, st, a);
}

// perm: ray order to bundle by (render mode), or NULL for the given order
int eslam_scatter_v2(const eslam_plane_t* planes, const Bound& bnd, const float* rays_o, const float* rays_d,
                     const float* z_or_pts, int64_t R, int S, bool render, const float* g_feat, const int* perm,
                     hipStream_t st, const DecReduceArgs* red, const eslam_decoders_t* gz_dec) {
    const int64_t N = render ? R * S : R;
    const bool gz = gz_dec != nullptr, det = eslam_deterministic();
    if (int rc = scatter_check_limits(planes, N, render, gz, red != nullptr)) return rc;
    const ScatterPlan plan = scatter_plan(planes, render ? S : 64, render ? (int)R : (int)((N + 63) / 64), gz, red != nullptr);
    g_last_scatter_paired = plan.paired ? 1 : 0;

    ScatterArgs a = {};
    for (int i = 0; i < NPL; ++i) a.planes.p[i] = planes[i];
    a.bnd = bnd;
    a.rays_o = rays_o;
    a.rays_d = rays_d;
    a.z_or_pts = z_or_pts;
    a.perm = render ? perm : nullptr;
    a.R = (int)R;
    a.S = render ? S : 64;
    a.g_feat = g_feat;
    a.bundle = plan.bundle;
    a.nbundles = plan.nbundles;
    a.work = plan.work;
    if (red) a.red = *red;
    a.red_blocks = plan.red_blocks;
    if (gz) { a.gz_w1_sdf = gz_dec->w1; a.gz_w1_rgb = gz_dec->cw1; }

    if (det) {
        // fixed-point scatter into the int64 shadow, then shadow -> float gradients (DET in eslam_scatter_dev.h)
        if (int rc = scatter_shadow(planes, st, &a.shadow, &a.shoff)) return rc;
        if (render) scatter_launch<true, true, 4, false, false>(a, plan.grid, st);
        else scatter_launch<false, true, 4, false, false>(a, plan.grid, st);
        if (int rc = eslam_check_launch("scatter_sort_kernel<det>")) return rc;
        for (int i = 0; i < NPL; ++i) {
            const int64_t numel = (int64_t)ESLAM_C_DIM * planes[i].h * planes[i].w;
            hipLaunchKernelGGL(scatter_fixed_to_float_kernel, dim3((unsigned)((numel + 255) / 256 < 2048 ? (numel + 255) / 256 : 2048)),
                               dim3(256), 0, st, planes[i].grad, a.shadow + a.shoff.o[i], numel);
        }
        return eslam_check_launch("scatter_fixed_to_float_kernel");
    }
    const bool small = plan.bm == 1024;
    if (gz && plan.paired) {
        if (small) scatter_launch<true, false, 2, true, true>(a, plan.grid, st);
        else scatter_launch<true, false, 4, true, true>(a, plan.grid, st);
    } else if (gz) {
        if (small) scatter_launch<true, false, 2, true, false>(a, plan.grid, st);
        else scatter_launch<true, false, 4, true, false>(a, plan.grid, st);
    } else if (render) {
        if (small) scatter_launch<true, false, 2, false, false>(a, plan.grid, st);
        else scatter_launch<true, false, 4, false, false>(a, plan.grid, st);
    } else {
        if (small) scatter_launch<false, false, 2, false, false>(a, plan.grid, st);
        else scatter_launch<false, false, 4, false, false>(a, plan.grid, st);
    }
    return eslam_check_launch("scatter_sort_kernel");
}
