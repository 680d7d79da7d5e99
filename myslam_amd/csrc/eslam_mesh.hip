// Marching cubes on a float32 volume [nx][ny][nz] (z fastest): replaces skimage.measure.marching_cubes in reference
// src/utils/Mesher.py:222-239.  Welded vertices (one per crossing edge) and faces in a fixed order, so the output is
// deterministic and can be compared bit for bit.  Cube and edge numbering: eslam_mc_tables.h (tools/gen_mc_tables.py).
//
// Three passes over chunks of MC_CHUNK consecutive grid points (thread t of a chunk takes points t, t + 256, ...):
//   count  per point: the crossing bits of its +x, +y, +z edges and the case of the cube it is the lower corner of,
//          kept in the workspace (1 byte each); per chunk: vertex and face totals;
//   scan   one workgroup: exclusive scan of the chunk totals (in place), grand totals to the caller;
//   emit   vertices (and the index of each point's first vertex), then faces, each at its chunk's offset plus an
//          in-chunk scan in point order.
#define MC_TABLE __constant__ static const
#include "eslam_common.h"
#include "eslam_mc_tables.h"

#define MC_THREADS 256
#define MC_PER_THREAD 16
#define MC_CHUNK (MC_THREADS * MC_PER_THREAD)
#define MC_SCAN_THREADS 1024

struct McGrid {
    int64_t nx, ny, nz, sx, N;     // sx = ny * nz: the x stride
};

__device__ __forceinline__ void mc_coords(const McGrid& g, int64_t i, int64_t& ix, int64_t& iy, int64_t& iz) {
    if (g.N <= (int64_t)0xffffffffu) {        // 32-bit divisions when every index fits
        const uint32_t ii = (uint32_t)i, nz = (uint32_t)g.nz, ny = (uint32_t)g.ny;
        const uint32_t row = ii / nz;
        iz = ii - row * nz;
        ix = row / ny;
        iy = row - (uint32_t)ix * ny;
    } else {
        const int64_t row = i / g.nz;
        iz = i - row * g.nz;
        ix = row / g.ny;
        iy = row - ix * g.ny;
    }
}

// vertex id of edge `e` (0..11) of the cube whose lower corner is point i
__device__ __forceinline__ int mc_edge_vertex(const McGrid& g, int64_t i, int e, const int32_t* __restrict__ vbase,
                                              const uint8_t* __restrict__ ebits) {
    const int axis = e >> 2, j = e & 3;
    const int a = j & 1, b = j >> 1;
    const int64_t owner = axis == 0 ? i + a * g.nz + b : axis == 1 ? i + a * g.sx + b : i + a * g.sx + b * g.nz;
    return vbase[owner] + __popc((unsigned)ebits[owner] & ((1u << axis) - 1u));
}

// masked mode: the cube with lower corner (ix, iy, iz) exists and all eight of its corners were observed (weight > 0)
__device__ __forceinline__ bool mc_cube_valid(const float* __restrict__ weight, const McGrid& g, int64_t ix, int64_t iy,
                                              int64_t iz) {
    if (ix < 0 || iy < 0 || iz < 0 || ix + 1 >= g.nx || iy + 1 >= g.ny || iz + 1 >= g.nz) return false;
    const float* w = weight + (ix * g.ny + iy) * g.nz + iz;
    return w[0] > 0.0f && w[1] > 0.0f && w[g.nz] > 0.0f && w[g.nz + 1] > 0.0f && w[g.sx] > 0.0f && w[g.sx + 1] > 0.0f &&
           w[g.sx + g.nz] > 0.0f && w[g.sx + g.nz + 1] > 0.0f;
}

// MASKED (eslam_mc_count_masked): a cube keeps its case only when it is valid, an edge its crossing bit only when one of
// the (up to four) cubes around it is; the emit kernels read nothing but these bytes, so they serve both modes
template <bool MASKED>
__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float* __restrict__ vol, const float* __restrict__ weight,
                                                              const McGrid g, const float level,
                                                              uint8_t* __restrict__ ebits, uint8_t* __restrict__ cases,
                                                              int64_t* __restrict__ chunk_counts) {
    __shared__ int lds[MC_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * MC_CHUNK;
    int nv = 0, nf = 0;
    for (int k = 0; k < MC_PER_THREAD; ++k) {
        const int64_t i = c0 + k * MC_THREADS + threadIdx.x;
        if (i >= g.N) break;
        int64_t ix, iy, iz;
        mc_coords(g, i, ix, iy, iz);
        const bool hx = ix + 1 < g.nx, hy = iy + 1 < g.ny, hz = iz + 1 < g.nz;
        const bool b0 = vol[i] < level;
        const bool bx = hx ? vol[i + g.sx] < level : b0;
        const bool by = hy ? vol[i + g.nz] < level : b0;
        const bool bz = hz ? vol[i + 1] < level : b0;
        int e = (int)(bx != b0) | ((int)(by != b0) << 1) | ((int)(bz != b0) << 2);
        int cube = 0;
        if (MASKED && e) {
            // the cubes around the edge along axis a: lower corners at the point minus 0 or 1 along the two other axes
            const bool v00 = mc_cube_valid(weight, g, ix, iy, iz);
            int keep = 0;
            if (e & 1) keep |= (int)(v00 || mc_cube_valid(weight, g, ix, iy - 1, iz) || mc_cube_valid(weight, g, ix, iy, iz - 1) ||
                                     mc_cube_valid(weight, g, ix, iy - 1, iz - 1));
            if (e & 2) keep |= (int)(v00 || mc_cube_valid(weight, g, ix - 1, iy, iz) || mc_cube_valid(weight, g, ix, iy, iz - 1) ||
                                     mc_cube_valid(weight, g, ix - 1, iy, iz - 1)) << 1;
            if (e & 4) keep |= (int)(v00 || mc_cube_valid(weight, g, ix - 1, iy, iz) || mc_cube_valid(weight, g, ix, iy - 1, iz) ||
                                     mc_cube_valid(weight, g, ix - 1, iy - 1, iz)) << 2;
            e = keep;
        }
        if (hx && hy && hz && (!MASKED || mc_cube_valid(weight, g, ix, iy, iz))) {
            const bool bxy = vol[i + g.sx + g.nz] < level, bxz = vol[i + g.sx + 1] < level;
            const bool byz = vol[i + g.nz + 1] < level, bxyz = vol[i + g.sx + g.nz + 1] < level;
            cube = (int)b0 | ((int)bx << 1) | ((int)by << 2) | ((int)bxy << 3) | ((int)bz << 4) | ((int)bxz << 5) |
                   ((int)byz << 6) | ((int)bxyz << 7);
        }
        ebits[i] = (uint8_t)e;
        cases[i] = (uint8_t)cube;
        nv += __popc((unsigned)e);
        nf += MC_NTRI[cube];
    }
    int tv, tf;
    (void)block_excl_scan<int, MC_THREADS>(nv, lds, tv);
    (void)block_excl_scan<int, MC_THREADS>(nf, lds, tf);
    if (threadIdx.x == 0) {
        chunk_counts[2 * blockIdx.x] = tv;
        chunk_counts[2 * blockIdx.x + 1] = tf;
    }
}

// one workgroup: chunk (vertex, face) totals -> exclusive offsets, in place; totals[0..1] = (n_verts, n_faces)
__global__ __launch_bounds__(MC_SCAN_THREADS) void mc_scan_kernel(int64_t* __restrict__ chunk_counts, int64_t nchunks,
                                                                  int64_t* __restrict__ totals) {
    __shared__ int64_t lds[MC_SCAN_THREADS / 64];
    int64_t carry_v = 0, carry_f = 0;
    for (int64_t base = 0; base < nchunks; base += MC_SCAN_THREADS) {
        const int64_t c = base + threadIdx.x;
        const int64_t v = c < nchunks ? chunk_counts[2 * c] : 0, f = c < nchunks ? chunk_counts[2 * c + 1] : 0;
        int64_t tv, tf;
        const int64_t ev = block_excl_scan<int64_t, MC_SCAN_THREADS>(v, lds, tv);
        const int64_t ef = block_excl_scan<int64_t, MC_SCAN_THREADS>(f, lds, tf);
        if (c < nchunks) {
            chunk_counts[2 * c] = carry_v + ev;
            chunk_counts[2 * c + 1] = carry_f + ef;
        }
        carry_v += tv;
        carry_f += tf;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_v;
        totals[1] = carry_f;
    }
}

struct McFrame {
    double origin[3], spacing[3];
};

__global__ __launch_bounds__(MC_THREADS) void mc_emit_verts_kernel(const float* __restrict__ vol, const McGrid g, const float level,
                                                                   const McFrame fr, const uint8_t* __restrict__ ebits,
                                                                   const int64_t* __restrict__ chunk_counts,
                                                                   int32_t* __restrict__ vbase, float* __restrict__ verts) {
    __shared__ int lds[MC_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * MC_CHUNK;
    int64_t next = chunk_counts[2 * blockIdx.x];
    for (int k = 0; k < MC_PER_THREAD; ++k) {
        if (c0 + k * MC_THREADS >= g.N) break;                 // (uniform over the workgroup)
        const int64_t i = c0 + k * MC_THREADS + threadIdx.x;
        const int e = i < g.N ? ebits[i] : 0;
        const int nv = __popc((unsigned)e);
        int tot;
        const int off = block_excl_scan<int, MC_THREADS>(nv, lds, tot);
        if (nv) {
            int64_t vid = next + off;
            vbase[i] = (int32_t)vid;
            int64_t ix, iy, iz;
            mc_coords(g, i, ix, iy, iz);
            const int64_t idx[3] = {ix, iy, iz};
            const int64_t stride[3] = {g.sx, g.nz, 1};
            const double lo = vol[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!((e >> a) & 1)) continue;
                const double hi = vol[i + stride[a]];
                // exactly one end is below the level, so hi != lo; a corner equal to the level gives t = 0 or 1
                const double t = ((double)level - lo) / (hi - lo);
                float* out = verts + vid * 3;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double pos = (double)idx[d] + (d == a ? t : 0.0);
                    out[d] = (float)(fr.origin[d] + pos * fr.spacing[d]);
                }
                ++vid;
            }
        }
        next += tot;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_faces_kernel(const McGrid g, const uint8_t* __restrict__ ebits,
                                                                   const uint8_t* __restrict__ cases,
                                                                   const int64_t* __restrict__ chunk_counts,
                                                                   const int32_t* __restrict__ vbase,
                                                                   int32_t* __restrict__ faces) {
    __shared__ int lds[MC_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * MC_CHUNK;
    int64_t next = chunk_counts[2 * blockIdx.x + 1];
    for (int k = 0; k < MC_PER_THREAD; ++k) {
        if (c0 + k * MC_THREADS >= g.N) break;
        const int64_t i = c0 + k * MC_THREADS + threadIdx.x;
        const int cube = i < g.N ? cases[i] : 0;
        const int nf = MC_NTRI[cube];
        int tot;
        const int off = block_excl_scan<int, MC_THREADS>(nf, lds, tot);
        int32_t* out = faces + (next + off) * 3;
        for (int t = 0; t < 3 * nf; ++t) out[t] = mc_edge_vertex(g, i, MC_TRI[cube][t], vbase, ebits);
        next += tot;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static int64_t mc_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static bool mc_grid(const char* who, int64_t nx, int64_t ny, int64_t nz, McGrid& g) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > ((int64_t)1 << 40) / ny / nz) {
        eslam_set_error("%s: grid %lld x %lld x %lld is empty or too large", who, (long long)nx, (long long)ny, (long long)nz);
        return false;
    }
    g.nx = nx; g.ny = ny; g.nz = nz; g.sx = ny * nz; g.N = nx * ny * nz;
    return true;
}

static int64_t mc_chunks(int64_t N) { return (N + MC_CHUNK - 1) / MC_CHUNK; }

extern "C" int64_t eslam_mc_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > ((int64_t)1 << 40) / ny / nz) return -1;
    const int64_t N = nx * ny * nz;
    return mc_align(16 * mc_chunks(N)) + mc_align(4 * N) + 2 * mc_align(N);
}

struct McWork {
    int64_t* chunk_counts;
    int32_t* vbase;
    uint8_t* ebits;
    uint8_t* cases;
};

static McWork mc_work(void* ws, int64_t N) {
    char* p = (char*)ws;
    McWork w;
    w.chunk_counts = (int64_t*)p;
    p += mc_align(16 * mc_chunks(N));
    w.vbase = (int32_t*)p;
    p += mc_align(4 * N);
    w.ebits = (uint8_t*)p;
    p += mc_align(N);
    w.cases = (uint8_t*)p;
    return w;
}

template <bool MASKED>
static int mc_count(const char* who, const float* vol, const float* weight, int64_t nx, int64_t ny, int64_t nz, float level,
                    void* workspace, int64_t* counts, eslam_stream_t stream) {
    McGrid g;
    if (!mc_grid(who, nx, ny, nz, g)) return 1;
    if (!vol || !workspace || !counts || (MASKED && !weight)) {
        eslam_set_error("%s: null argument", who);
        return 1;
    }
    const McWork w = mc_work(workspace, g.N);
    const int64_t nch = mc_chunks(g.N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_count_kernel<MASKED>, dim3((unsigned)nch), dim3(MC_THREADS), 0, st, vol, weight, g, level, w.ebits,
                       w.cases, w.chunk_counts);
    if (eslam_check_launch("mc_count_kernel")) return 1;
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.chunk_counts, nch, counts);
    return eslam_check_launch("mc_scan_kernel");
}

extern "C" int eslam_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace,
                              int64_t* counts, eslam_stream_t stream) {
    return mc_count<false>("eslam_mc_count", vol, nullptr, nx, ny, nz, level, workspace, counts, stream);
}

extern "C" int eslam_mc_count_masked(const float* vol, const float* weight, int64_t nx, int64_t ny, int64_t nz, float level,
                                     void* workspace, int64_t* counts, eslam_stream_t stream) {
    return mc_count<true>("eslam_mc_count_masked", vol, weight, nx, ny, nz, level, workspace, counts, stream);
}

extern "C" int eslam_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, float level, const double* origin3_host,
                             const double* spacing3_host, const void* workspace, int64_t n_verts, int64_t n_faces,
                             float* verts, int32_t* faces, eslam_stream_t stream) {
    McGrid g;
    if (!mc_grid("eslam_mc_emit", nx, ny, nz, g)) return 1;
    if (n_verts < 0 || n_faces < 0) {
        eslam_set_error("eslam_mc_emit: negative counts");
        return 1;
    }
    if (n_verts > INT32_MAX) {
        eslam_set_error("eslam_mc_emit: %lld vertices exceed the int32 face indices (2^31 - 1 at most)", (long long)n_verts);
        return 1;
    }
    if (!vol || !workspace || !origin3_host || !spacing3_host || (n_verts && !verts) || (n_faces && !faces)) {
        eslam_set_error("eslam_mc_emit: null argument");
        return 1;
    }
    if (n_verts == 0) return 0;
    McFrame fr;
    for (int d = 0; d < 3; ++d) {
        fr.origin[d] = origin3_host[d];
        fr.spacing[d] = spacing3_host[d];
    }
    const McWork w = mc_work(const_cast<void*>(workspace), g.N);
    const int64_t nch = mc_chunks(g.N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_emit_verts_kernel, dim3((unsigned)nch), dim3(MC_THREADS), 0, st, vol, g, level, fr, w.ebits,
                       w.chunk_counts, w.vbase, verts);
    if (eslam_check_launch("mc_emit_verts_kernel")) return 1;
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(mc_emit_faces_kernel, dim3((unsigned)nch), dim3(MC_THREADS), 0, st, g, w.ebits, w.cases,
                       w.chunk_counts, w.vbase, faces);
    return eslam_check_launch("mc_emit_faces_kernel");
}
