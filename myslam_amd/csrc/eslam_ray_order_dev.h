// The ray ordering and the gradient clear as device functions: the bodies of ray_order_kernel (eslam_ray_order.hip) and of the
// ordering / clear roles of step_front_kernel (eslam_sample.hip).  The two files are compiled with different -ffp-contract
// settings, so the ordering pins its own (contraction ON, as ray_order_kernel has always been compiled): its keys and the fan
// extents come out the same from either file.
#pragma once
#include "eslam_common.h"

#define SORT_MAX 8192

__device__ __forceinline__ unsigned spread3(unsigned v) {      // 10 bits -> every third bit
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// One workgroup orders one chunk of up to SORT_MAX rays with a single-pass counting sort in LDS:
// key = 15-bit Morton code of the point one metre along the ray, quantised inside the chunk's bounding box of such
// points (rays of one camera: a patch of the unit sphere round its centre; several cameras: several patches, and
// rays of nearby cameras with similar directions end up adjacent, which is what shares texels).  Order inside a cell
// is arbitrary (atomic tickets).  perm[chunk*SORT_MAX + i] = ray id.  (A 78-stage bitonic network in one workgroup took
// 62 us for 4096 rays; this kernel's time is in DESIGN.md section 5.)
// When all rays of the chunk leave from ONE point (a tracking batch; a mapping batch of a single frame) their
// directions form a 2-D patch, and a 3-D Morton code wastes a third of its bits on a coordinate the other two
// determine: the key is then the azimuth of the direction projected into the order's plane (see below).  Round 2's
// 16-bit Hilbert index of the direction's gnomonic projection, one order for all planes, had measured 14 % fewer cell
// flushes than the Morton code on the bench workload (scatter 124 -> 116 us; tools/sim_order.py, tools/exp_order.py).
#define ORD_BITS 5
#define ORD_CELLS (1 << (3 * ORD_BITS))      // 32768 words = 65536 packed 16-bit counters = 128 KB of LDS
#define ORD_PER_THREAD (SORT_MAX / 1024)
// key_bits (12 or 14): keys of the counting sort.  The histogram's zero fill and scan are what the single workgroup
// spends its time on, so small batches get short keys (12 bits for <= 1024 rays: 2048 words instead of 8192).
// (16-bit keys were for the 2-D Hilbert order of round 2: 8 bits per axis.  The azimuth keys are one-dimensional: 14 bits = two
// bins per ray at 8192 rays, and the histogram's zero fill and scan - 63 us of this kernel at 5000 rays with 16 bits - shrink 4x)
static inline int ray_order_key_bits(int R) { return (R < SORT_MAX ? R : SORT_MAX) <= 1024 ? 12 : 14; }
static inline size_t ray_order_hist_bytes(int key_bits) { return ((size_t)1 << key_bits) / 2 * sizeof(unsigned); }
// dynamic LDS of an ordering workgroup: the histogram and, behind it, the chunk's sorted ray ids (16 bits each)
static inline size_t ray_order_lds_bytes(int key_bits) { return ray_order_hist_bytes(key_bits) + SORT_MAX * sizeof(unsigned short); }
static inline int ray_order_blocks(int R) { return R > 0 ? (R + SORT_MAX - 1) / SORT_MAX * ESLAM_RAY_ORDERS : 0; }
// clearing workgroups: one per 64 KB, at most one per CU of a 256-CU chip (each then stores 16 KB per trip)
static inline int ray_clear_blocks(int64_t clear_bytes) {
    const int64_t want = (clear_bytes + 65535) / 65536;
    return (int)(want < 256 ? want : 256);
}
// the argument checks of a launch that orders R rays and zeroes clear_bytes at `clear` (1: refused, the message is set)
static inline int ray_order_check_args(const char* who, const float* rays_o, const float* rays_d, int R, const int32_t* perm,
                                       const void* clear, int64_t clear_bytes) {
    if (clear_bytes < 0 || (clear_bytes > 0 && !clear) || ((uintptr_t)clear & 15) || (clear_bytes & 3)) {
        eslam_set_error("%s: the buffer to clear must be 16-byte aligned and a multiple of 4 bytes long (%p, %lld bytes)", who, clear,
                        (long long)clear_bytes);
        return 1;
    }
    if (R > 0 && (!rays_o || !rays_d || !perm)) {
        eslam_set_error("%s: null argument", who);
        return 1;
    }
    return 0;
}

// Clearing workgroup `block` of `nblocks` (1024 threads each): zero clear_words floats at `clear` (16-byte aligned) with
// 16-byte stores.
__device__ __forceinline__ void ray_clear_block(float* __restrict__ clear, const long long clear_words, const int block,
                                                const int nblocks) {
    const long long n16 = clear_words >> 2;
    const long long stride = (long long)nblocks * 1024;
    float4_t* const c4 = (float4_t*)clear;
    const float4_t z4 = {0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)block * 1024 + threadIdx.x; i < n16; i += stride) c4[i] = z4;
    if (block == 0 && (long long)threadIdx.x < (clear_words & 3)) clear[4 * n16 + threadIdx.x] = 0.f;
}

// Ordering workgroup `block` (1024 threads): chunk block / ESLAM_RAY_ORDERS, orientation block % ESLAM_RAY_ORDERS.
// hist: ray_order_lds_bytes(key_bits) of LDS, 16-byte aligned: [(1 << key_bits) / 2] words of packed 16-bit counters, then the ids.
__device__ __forceinline__ void ray_order_block(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const int R,
                                                int* __restrict__ perm, const int key_bits, const int block, unsigned* const hist) {
#pragma clang fp contract(fast)
    const int chunk = block / ESLAM_RAY_ORDERS;
    const int nwords = (1 << key_bits) >> 1;
    const int mbits = key_bits / 3;                                       // Morton grid: 2^mbits per axis
    __shared__ float red[16][6];
    __shared__ float red2[16][11];
    __shared__ unsigned wsum[16];
    // several origins (a keyframe window, src/Mapper.py:308-319: the batch is camera-major): which rays start a new camera
    // (bit i of the map: ray i leaves from another point than ray i - 1), the running count per 64 rays, and per camera the sum
    // of its directions and the extent of its fan in this plane
    constexpr int NCAM_MAX = 32;
    __shared__ unsigned long long cam_bits[SORT_MAX / 64];
    __shared__ unsigned cam_before[SORT_MAX / 64 + 1];
    __shared__ float cam_dir[NCAM_MAX][3];
    __shared__ unsigned cam_ext[NCAM_MAX][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < SORT_MAX / 64) cam_bits[tid] = 0ull;
    if (tid < NCAM_MAX) { cam_dir[tid][0] = cam_dir[tid][1] = cam_dir[tid][2] = 0.f; cam_ext[tid][0] = 0xFFFFFFFFu; cam_ext[tid][1] = 0u; }
    __syncthreads();
    const int base = chunk * SORT_MAX;
    const int n = min(SORT_MAX, R - base);
    // orientation (0: xy, 1: xz, 2: yz): order number o is written to perm + o * R.  When the rays share one
    // origin, order o sorts them by the AZIMUTH of their direction projected into plane o: the rays of a bundle then lie on top
    // of each other in that plane's projection whatever their angle out of it, and that is what shares cells - a plane collapses
    // one axis, so a square patch of the image (round 2's Hilbert order: one order for all planes) spreads over many more cells of
    // each plane than a thin wedge does.  tools/sim_order.py, bench rays: 58.8 k cell flushes against 135 k.
    const int orient = block % ESLAM_RAY_ORDERS;
    float* const fan = (float*)(perm + (size_t)ESLAM_RAY_ORDERS * R);      // [ESLAM_RAY_ORDERS] angular extent of the fan in each plane (0: unknown)
    perm += (size_t)orient * R;
    const int pa = orient == 2 ? 1 : 0, pb = orient == 0 ? 1 : 2;       // the plane's two axes

    // Every thread reads its rays ONCE, four at a time with all of the loads in flight together, and keeps their unit directions'
    // two components in this order's plane (16 registers) for the single-origin branch below.  The other two branches re-read them from memory (98 KB, cache
    // resident) through unit_dir instead: at 1024 threads per workgroup the budget is 128 VGPRs, and round 2's Hilbert path spilled.
    auto normalise = [](float dx, float dy, float dz, float d[3]) {
#pragma clang fp contract(fast)
        const float inv = rsqrtf(fmaxf(dx * dx + dy * dy + dz * dz, 1e-20f));
        d[0] = dx * inv; d[1] = dy * inv; d[2] = dz * inv;
    };
    auto unit_dir = [&](int ray, float o[3], float d[3]) {
        normalise(rays_d[3 * ray], rays_d[3 * ray + 1], rays_d[3 * ray + 2], d);
        o[0] = rays_o[3 * ray]; o[1] = rays_o[3 * ray + 1]; o[2] = rays_o[3 * ray + 2];
    };
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    float olo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, ohi[3] = {-3.4e38f, -3.4e38f, -3.4e38f}, dsum[3] = {0.f, 0.f, 0.f};
    float ua[ORD_PER_THREAD], ub[ORD_PER_THREAD];           // components pa, pb of the unit directions
    static_assert(ORD_PER_THREAD % 4 == 0, "rays are read four per thread at a time");
#pragma unroll
    for (int k0 = 0; k0 < ORD_PER_THREAD; k0 += 4) {
        float ro[4][3], rd[4][3], rp[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int a = 0; a < 3; ++a) ro[k][a] = rd[k][a] = rp[k][a] = 0.f;
            ua[k0 + k] = ub[k0 + k] = 0.f;
        }
        if (k0 * 1024 >= n) continue;                         // (uniform over the workgroup)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + (k0 + k) * 1024;
            if (i < n) {
                const float* po = rays_o + 3 * (size_t)(base + i);
                const float* pd = rays_d + 3 * (size_t)(base + i);
#pragma unroll
                for (int a = 0; a < 3; ++a) { ro[k][a] = po[a]; rd[k][a] = pd[a]; }
                // the ray in front (which rays start a new camera): the neighbouring lane's, read from memory by lane 0 only
                if (lane == 0 && i > 0) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) rp[k][a] = po[a - 3];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + (k0 + k) * 1024;
            float prev[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {                     // (outside the branch: every lane of the wave takes part)
                const float up = __shfl_up(ro[k][a], 1, WAVE);
                prev[a] = lane == 0 ? rp[k][a] : up;
            }
            if (i < n) {
                float d[3];
                normalise(rd[k][0], rd[k][1], rd[k][2], d);
                const float* o = ro[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    olo[a] = fminf(olo[a], o[a]); ohi[a] = fmaxf(ohi[a], o[a]);
                    dsum[a] += d[a];
                    const float p = o[a] + d[a];
                    lo[a] = fminf(lo[a], p); hi[a] = fmaxf(hi[a], p);
                }
                ua[k0 + k] = orient == 2 ? d[1] : d[0];
                ub[k0 + k] = orient == 0 ? d[1] : d[2];
                const bool first = i == 0 || prev[0] != o[0] || prev[1] != o[1] || prev[2] != o[2];
                const unsigned long long fb = __ballot(first);          // (a wave's rays of one trip are 64 consecutive ones)
                if (lane == 0) cam_bits[i >> 6] = fb;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m, WAVE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m, WAVE));
            olo[a] = fminf(olo[a], __shfl_xor(olo[a], m, WAVE));
            ohi[a] = fmaxf(ohi[a], __shfl_xor(ohi[a], m, WAVE));
            dsum[a] += __shfl_xor(dsum[a], m, WAVE);
        }
        if (lane == 0) {
            red[wave][a] = lo[a]; red[wave][3 + a] = hi[a];
            red2[wave][a] = olo[a]; red2[wave][3 + a] = ohi[a]; red2[wave][6 + a] = dsum[a];
        }
    }
    for (int i = tid; i < nwords; i += 1024) hist[i] = 0u;
    __syncthreads();
    // cameras of the chunk: running count of "first ray of a camera" bits in front of every 64-ray word
    if (wave == 0) {
        constexpr int NW = SORT_MAX / 64;                        // 128 words: two per lane
        const unsigned c0 = __popcll(cam_bits[2 * lane]), c1 = __popcll(cam_bits[2 * lane + 1]);
        const unsigned incl = wave_incl_sum_u(c0 + c1);
        cam_before[2 * lane] = incl - c0 - c1;
        cam_before[2 * lane + 1] = incl - c1;
        if (lane == 63) cam_before[NW] = incl;
    }
    __syncthreads();
    const int ncam = (int)cam_before[SORT_MAX / 64];
    auto camera_of = [&](int i) {                                // 0-based camera of ray i of the chunk
        const unsigned long long below = cam_bits[i >> 6] & (~0ull >> (63 - (i & 63)));
        return (int)(cam_before[i >> 6] + (unsigned)__popcll(below)) - 1;
    };
    auto sortable = [](float x) { const unsigned u = __float_as_uint(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    auto unsortable = [](unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); };
    const bool per_camera = ncam >= 2 && ncam <= NCAM_MAX;
    // one origin?  then order by the azimuth of the direction about the mean direction
    float mdir[3];
    bool single = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = red2[0][a], h = red2[0][3 + a], sm = red2[0][6 + a];
        for (int w = 1; w < 16; ++w) { l = fminf(l, red2[w][a]); h = fmaxf(h, red2[w][3 + a]); sm += red2[w][6 + a]; }
        mdir[a] = sm;
        single = single && (h - l) <= 1e-6f * fmaxf(1.0f, fabsf(h));
    }
    const float mlen = sqrtf(mdir[0] * mdir[0] + mdir[1] * mdir[1] + mdir[2] * mdir[2]);
    single = single && mlen > 0.5f * (float)n;          // a usable mean direction (field of view well below 180 degrees)
    unsigned key[ORD_PER_THREAD], ticket[ORD_PER_THREAD];
#pragma unroll
    for (int k = 0; k < ORD_PER_THREAD; ++k) { key[k] = 0; ticket[k] = 0; }
    if (per_camera) {                                   // uniform over the workgroup
        // A keyframe window: key = (camera, azimuth of the direction projected into this plane, measured against the camera's own
        // projected mean direction) - each camera's rays form thin wedges of the plane, as the single camera's do below.
        // tools/sim_order_window.py (10 cameras x 400 rays x 40): 211 k cell flushes against 338 k for the Morton order.
        for (int i = tid; i < n; i += 1024) {
            float o[3], d[3];
            unit_dir(base + i, o, d);
            const int c = camera_of(i);
            atomicAdd(&cam_dir[c][0], d[0]); atomicAdd(&cam_dir[c][1], d[1]); atomicAdd(&cam_dir[c][2], d[2]);
        }
        __syncthreads();
        auto angle = [&](int i, int& c) {
#pragma clang fp contract(fast)
            float o[3], d[3];
            unit_dir(base + i, o, d);
            c = camera_of(i);
            const float ma = cam_dir[c][pa], mb = cam_dir[c][pb];
            return atan2f(ma * d[pb] - mb * d[pa], ma * d[pa] + mb * d[pb]);
        };
        for (int i = tid; i < n; i += 1024) {
            int c;
            const unsigned u = sortable(angle(i, c));
            atomicMin(&cam_ext[c][0], u);
            atomicMax(&cam_ext[c][1], u);
        }
        __syncthreads();
        const int cbits = 32 - __clz(ncam - 1);          // bits for the camera (ncam >= 2)
        const int abits = key_bits - cbits;              // >= 7: key_bits >= 12, cbits <= 5
        if (tid == 0 && chunk == 0) fan[orient] = 0.0f;      // several origins: no single fan
#pragma unroll
        for (int k = 0; k < ORD_PER_THREAD; ++k) {
            const int i = tid + k * 1024;
            if (i < n) {
                int c;
                const float ang = angle(i, c);
                const float l = unsortable(cam_ext[c][0]), h = unsortable(cam_ext[c][1]);
                const unsigned amax = (1u << abits) - 1u;
                const unsigned qa = min((unsigned)fmaxf((ang - l) * ((float)(1u << abits) / fmaxf(h - l, 1e-6f)), 0.f), amax);
                const unsigned kk = ((unsigned)c << abits) | qa;
                key[k] = kk;
                ticket[k] = (atomicAdd(&hist[kk >> 1], 1u << ((kk & 1u) * 16u)) >> ((kk & 1u) * 16u)) & 0xFFFFu;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else if (single) {                                // uniform over the workgroup
        const float mpa = mdir[pa] / mlen, mpb = mdir[pb] / mlen;      // the mean direction projected into the plane
        // the signed angle between the projected direction and the projected mean: once per ray, kept for the key pass
        float az[ORD_PER_THREAD];
        float blo = 3.4e38f, bhi = -3.4e38f;
#pragma unroll
        for (int k = 0; k < ORD_PER_THREAD; ++k) {
            az[k] = 0.f;
            if (tid + k * 1024 < n) {
                az[k] = atan2f(mpa * ub[k] - mpb * ua[k], mpa * ua[k] + mpb * ub[k]);
                blo = fminf(blo, az[k]); bhi = fmaxf(bhi, az[k]);
            }
            __builtin_amdgcn_sched_barrier(0);           // one ray at a time keeps the register pressure down
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            blo = fminf(blo, __shfl_xor(blo, m, WAVE));
            bhi = fmaxf(bhi, __shfl_xor(bhi, m, WAVE));
        }
        if (lane == 0) { red2[wave][9] = blo; red2[wave][10] = bhi; }
        __syncthreads();
        float h = red2[0][10];
        blo = red2[0][9];
        for (int w = 1; w < 16; ++w) { blo = fminf(blo, red2[w][9]); h = fmaxf(h, red2[w][10]); }
        const float sc = (float)(1 << key_bits) / fmaxf(h - blo, 1e-6f);
        // the fan's angular extent in this plane (radians), for the scatter's choice of grid order; the first chunk speaks for the batch
        if (tid == 0 && chunk == 0) fan[orient] = h - blo;
#pragma unroll
        for (int k = 0; k < ORD_PER_THREAD; ++k) {
            const int i = tid + k * 1024;
            if (i < n) {
                const unsigned kk = min((unsigned)fmaxf((az[k] - blo) * sc, 0.f), (1u << key_bits) - 1u);
                key[k] = kk;
                ticket[k] = (atomicAdd(&hist[kk >> 1], 1u << ((kk & 1u) * 16u)) >> ((kk & 1u) * 16u)) & 0xFFFFu;
            }
        }
    } else {
        if (tid == 0 && chunk == 0) fan[orient] = 0.0f;      // several origins: no fan
        float scale[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = red[0][a], h = red[0][3 + a];
            for (int w = 1; w < 16; ++w) { l = fminf(l, red[w][a]); h = fmaxf(h, red[w][3 + a]); }
            lo[a] = l;
            scale[a] = (float)(1 << mbits) / fmaxf(h - l, 1e-6f);
        }
#pragma unroll
        for (int k = 0; k < ORD_PER_THREAD; ++k) {
            const int i = tid + k * 1024;
            if (i < n) {
                float o[3], d[3];
                unit_dir(base + i, o, d);
                const unsigned qmax = (1u << mbits) - 1;
                const unsigned qx = min((unsigned)fmaxf((o[0] + d[0] - lo[0]) * scale[0], 0.f), qmax);
                const unsigned qy = min((unsigned)fmaxf((o[1] + d[1] - lo[1]) * scale[1], 0.f), qmax);
                const unsigned qz = min((unsigned)fmaxf((o[2] + d[2] - lo[2]) * scale[2], 0.f), qmax);
                const unsigned kk = spread3(qx) | (spread3(qy) << 1) | (spread3(qz) << 2);
                key[k] = kk;
                ticket[k] = (atomicAdd(&hist[kk >> 1], 1u << ((kk & 1u) * 16u)) >> ((kk & 1u) * 16u)) & 0xFFFFu;
            }
        }
    }
    __syncthreads();
    // exclusive scan of the counters (two 16-bit counters per word, at most SORT_MAX = 8192 rays: no overflow):
    // thread t owns words [32t, 32t+32)
    const int per = nwords / 1024;                     // >= 2 (key_bits >= 12)
    // (a thread's 8 - or 2 - words leave and enter LDS as 16-byte (8-byte) accesses: word by word the stride of 8 words between
    // lanes is a 16-way bank conflict on each of 24 instructions, 2.1 us of the role at 4096 rays)
    unsigned local = 0;
    unsigned hw[8];
    if (per == 8) {
        const uint4 a = *(const uint4*)(hist + tid * 8), b = *(const uint4*)(hist + tid * 8 + 4);
        hw[0] = a.x; hw[1] = a.y; hw[2] = a.z; hw[3] = a.w; hw[4] = b.x; hw[5] = b.y; hw[6] = b.z; hw[7] = b.w;
    } else {
        const uint2 a = *(const uint2*)(hist + tid * 2);
        hw[0] = a.x; hw[1] = a.y;
#pragma unroll
        for (int j = 2; j < 8; ++j) hw[j] = 0u;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) local += (hw[j] & 0xFFFFu) + (hw[j] >> 16);
    unsigned incl = local;
#pragma unroll
    for (int dlt = 1; dlt < WAVE; dlt <<= 1) {
        const unsigned o = __shfl_up(incl, dlt, WAVE);
        if (lane >= dlt) incl += o;
    }
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    // the waves' bases: lane l < 16 reads wave l's sum once, an exclusive scan over the 16 lanes, wave w takes lane w's
    unsigned wpre = lane < 16 ? wsum[lane] : 0u;
    const unsigned wown = wpre;
#pragma unroll
    for (int dlt = 1; dlt < 16; dlt <<= 1) {
        const unsigned o = __shfl_up(wpre, dlt, WAVE);
        if (lane >= dlt) wpre += o;
    }
    const unsigned wbase = __shfl(wpre - wown, wave, WAVE);
    unsigned run = wbase + incl - local;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned c0 = hw[j] & 0xFFFFu, c1 = hw[j] >> 16;
        hw[j] = run | ((run + c0) << 16);
        run += c0 + c1;
    }
    if (per == 8) {
        *(uint4*)(hist + tid * 8) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        *(uint4*)(hist + tid * 8 + 4) = make_uint4(hw[4], hw[5], hw[6], hw[7]);
    } else {
        *(uint2*)(hist + tid * 2) = make_uint2(hw[0], hw[1]);
    }
    __syncthreads();
    // placement: the ray ids go to their places in LDS first (16 bits each, behind the histogram: ray_order_lds_bytes) and leave
    // as coalesced 4-byte stores; one scattered global store per ray was 0.7 us longer at 4096 rays
    unsigned short* const sorted = (unsigned short*)(hist + nwords);      // [n]
#pragma unroll
    for (int k = 0; k < ORD_PER_THREAD; ++k) {
        const int i = tid + k * 1024;
        if (i < n) {
            const unsigned start = (hist[key[k] >> 1] >> ((key[k] & 1u) * 16u)) & 0xFFFFu;
            sorted[start + ticket[k]] = (unsigned short)i;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORD_PER_THREAD; ++k) {
        const int i = tid + k * 1024;
        if (i < n) perm[base + i] = base + (int)sorted[i];
    }
}
