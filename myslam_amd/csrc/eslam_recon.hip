// Mesh culling and the 3D reconstruction metrics' search: replaces the per-frame visibility test of reference
// src/tools/cull_mesh.py:61-104 and the nearest-neighbour queries of src/tools/eval_recon.py:21-49 (scipy's
// cKDTree.query, open3d's ICP correspondence search), plus the ICP's correspondence moments.
//
//   cull     one launch per chunk of K frames: every vertex not yet seen is projected into the K frames (poses are
//            wave-uniform: scalar loads) and marked when one of them sees it;
//   nn       an exact nearest-neighbour search on a uniform grid of cubic cells.  Build: a counting sort of the
//            reference points into cell order (count with an atomic slot per point, exclusive scan, scatter) as
//            float4 (x, y, z, index bits).  Query: rings of cells around the query's (clamped) cell until the distance
//            to everything outside the searched box is at least the best so far; ties go to the smaller reference
//            index, so results do not depend on the order the atomics gave a cell's points.  Queries are processed in
//            cell order (the same counting sort) so that a wave's lanes walk the same cells;
//   moments  a fixed-order float64 reduction over the correspondences of one ICP round.
#include <math.h>

#include "eslam_common.h"

#define RC_THREADS 256
#define RC_PER_THREAD 16
#define RC_CHUNK (RC_THREADS * RC_PER_THREAD)       // scan chunk
#define RC_SCAN_THREADS 1024
#define RC_MAX_BLOCKS (1 << 20)                     // grid-stride loops beyond this many workgroups
#define ICP_BLOCKS 1024                             // partial sums of eslam_icp_moments (a constant: fixed order)

static int rc_blocks(int64_t n) {
    const int64_t b = (n + RC_THREADS - 1) / RC_THREADS;
    return (int)(b < 1 ? 1 : b > RC_MAX_BLOCKS ? RC_MAX_BLOCKS : b);
}

// ---------------------------------------------------------------------------------------------------------
// culling (cull_mesh.py:61-104)
// ---------------------------------------------------------------------------------------------------------
struct CullCam {
    float fx, fy, cx, cy, H, W, truncation;
    int depth_test;
};

// grid_sample(depth[None, None], grid, padding_mode='zeros', align_corners=True) at one point (x, y) in pixels:
// bilinear over the four neighbours, a neighbour outside the image contributes 0 (torch's nw, ne, sw, se order)
__device__ __forceinline__ float cull_sample(const float* __restrict__ img, int Hi, int Wi, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float x1f = x0f + 1.0f, y1f = y0f + 1.0f;
    const float w_nw = (x1f - x) * (y1f - y), w_ne = (x - x0f) * (y1f - y);
    const float w_sw = (x1f - x) * (y - y0f), w_se = (x - x0f) * (y - y0f);
    const bool in_x0 = x0 >= 0 && x0 < Wi, in_x1 = x0 + 1 >= 0 && x0 + 1 < Wi;
    const bool in_y0 = y0 >= 0 && y0 < Hi, in_y1 = y0 + 1 >= 0 && y0 + 1 < Hi;
    float d = 0.0f;
    if (in_x0 && in_y0) d += img[(int64_t)y0 * Wi + x0] * w_nw;
    if (in_x1 && in_y0) d += img[(int64_t)y0 * Wi + x0 + 1] * w_ne;
    if (in_x0 && in_y1) d += img[(int64_t)(y0 + 1) * Wi + x0] * w_sw;
    if (in_x1 && in_y1) d += img[(int64_t)(y0 + 1) * Wi + x0 + 1] * w_se;
    return d;
}

// One vertex per lane (grid-stride).  For frame k (w2c = inverse(c2w), float32 [3][4]), the reference's test:
//   1. c = w2c [p, 1]
//   2. a = fx (-c.x) + cx c.z,  b = fy c.y + cy c.z,  zz = c.z + 1e-5      (x flipped, K applied, cull_mesh.py:84-87)
//   3. u = a / zz,  v = b / zz
//   4. visible when -zz >= 0, 0 < u < W and 0 < v < H                   (edge = 0, cull_mesh.py:96-101)
//   5. with the depth test (eval_rec) also d + truncation >= -zz, d = the bilinear, zero-padded sample of the depth image
//      at pixel (u (Wi - 1) / W, v (Hi - 1) / H): grid_sample(align_corners=True) of grid 2 (u / W) - 1 (cull_mesh.py:89-93)
// k is uniform over the wave (the loop never exits early), so the pose is read with scalar loads.
__global__ __launch_bounds__(RC_THREADS) void cull_vertices_kernel(const float* __restrict__ verts, int64_t V,
                                                                   const float* __restrict__ depths, int K, int Hi, int Wi,
                                                                   const float* __restrict__ w2c, const CullCam cam,
                                                                   uint8_t* __restrict__ seen) {
    const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < V; i += stride) {
        if (seen[i]) continue;
        const float px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
        bool vis = false;
        for (int k = 0; k < K; ++k) {
            const float* m = w2c + 12 * k;
            const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
            const float m6 = m[6], m7 = m[7], m8 = m[8], m9 = m[9], m10 = m[10], m11 = m[11];
            if (vis) continue;
            const float cx_ = m0 * px + m1 * py + m2 * pz + m3;
            const float cy_ = m4 * px + m5 * py + m6 * pz + m7;
            const float cz_ = m8 * px + m9 * py + m10 * pz + m11;
            const float a = cam.fx * (-cx_) + cam.cx * cz_;
            const float b = cam.fy * cy_ + cam.cy * cz_;
            const float zz = cz_ + 1e-5f;
            const float u = a / zz, v = b / zz;
            bool ok = (-zz >= 0.0f) && (u < cam.W) && (u > 0.0f) && (v < cam.H) && (v > 0.0f);
            if (ok && cam.depth_test) {
                const float gx = 2.0f * (u / cam.W) - 1.0f, gy = 2.0f * (v / cam.H) - 1.0f;
                const float x = (gx + 1.0f) * 0.5f * (float)(Wi - 1), y = (gy + 1.0f) * 0.5f * (float)(Hi - 1);
                const float d = cull_sample(depths + (int64_t)k * Hi * Wi, Hi, Wi, x, y);
                ok = d + cam.truncation >= -zz;
            }
            vis = ok;
        }
        if (vis) seen[i] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// in-place exclusive scan of int32 a[0..n), total to a[n]: chunks of RC_CHUNK, the chunk totals, the offsets
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RC_THREADS) void rc_scan_chunks_kernel(int32_t* __restrict__ a, int64_t n,
                                                                    int32_t* __restrict__ partial) {
    __shared__ int32_t lds[RC_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * RC_CHUNK;
    int32_t next = 0;
    for (int k = 0; k < RC_PER_THREAD; ++k) {
        if (c0 + k * RC_THREADS >= n) break;                   // (uniform over the workgroup)
        const int64_t i = c0 + k * RC_THREADS + threadIdx.x;
        const int32_t v = i < n ? a[i] : 0;
        int32_t tot;
        const int32_t off = block_excl_scan<int32_t, RC_THREADS>(v, lds, tot);
        if (i < n) a[i] = next + off;
        next += tot;
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = next;
}

__global__ __launch_bounds__(RC_SCAN_THREADS) void rc_scan_partials_kernel(int32_t* __restrict__ partial, int64_t nchunks,
                                                                           int32_t* __restrict__ total) {
    __shared__ int32_t lds[RC_SCAN_THREADS / 64];
    int32_t carry = 0;
    for (int64_t base = 0; base < nchunks; base += RC_SCAN_THREADS) {
        const int64_t c = base + threadIdx.x;
        const int32_t v = c < nchunks ? partial[c] : 0;
        int32_t tot;
        const int32_t e = block_excl_scan<int32_t, RC_SCAN_THREADS>(v, lds, tot);
        if (c < nchunks) partial[c] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(RC_THREADS) void rc_scan_add_kernel(int32_t* __restrict__ a, int64_t n,
                                                                 const int32_t* __restrict__ partial) {
    const int64_t c0 = (int64_t)blockIdx.x * RC_CHUNK;
    const int32_t add = partial[blockIdx.x];
    for (int k = 0; k < RC_PER_THREAD; ++k) {
        const int64_t i = c0 + k * RC_THREADS + threadIdx.x;
        if (i < n) a[i] += add;
    }
}

static int64_t rc_chunks(int64_t n) { return (n + RC_CHUNK - 1) / RC_CHUNK; }

static int rc_scan(int32_t* a, int64_t n, int32_t* partial, hipStream_t st) {
    const int64_t nch = rc_chunks(n);
    hipLaunchKernelGGL(rc_scan_chunks_kernel, dim3((unsigned)nch), dim3(RC_THREADS), 0, st, a, n, partial);
    if (eslam_check_launch("rc_scan_chunks_kernel")) return 1;
    hipLaunchKernelGGL(rc_scan_partials_kernel, dim3(1), dim3(RC_SCAN_THREADS), 0, st, partial, nch, a + n);
    if (eslam_check_launch("rc_scan_partials_kernel")) return 1;
    hipLaunchKernelGGL(rc_scan_add_kernel, dim3((unsigned)nch), dim3(RC_THREADS), 0, st, a, n, partial);
    return eslam_check_launch("rc_scan_add_kernel");
}

// ---------------------------------------------------------------------------------------------------------
// nearest neighbours on a uniform grid
// ---------------------------------------------------------------------------------------------------------
struct NnDev {
    float lox, loy, loz, cell, inv;
    int nx, ny, nz;
};

__device__ __forceinline__ int nn_axis_cell(float p, float lo, float inv, int n) {
    // clamped in float first: queries far outside the box (or NaN, which fmaxf turns into 0) stay in range
    const float f = fminf(fmaxf(floorf((p - lo) * inv), 0.0f), (float)(n - 1));
    return (int)f;
}

__device__ __forceinline__ int nn_cell_of(const NnDev& g, float x, float y, float z) {
    const int ix = nn_axis_cell(x, g.lox, g.inv, g.nx), iy = nn_axis_cell(y, g.loy, g.inv, g.ny);
    const int iz = nn_axis_cell(z, g.loz, g.inv, g.nz);
    return (ix * g.ny + iy) * g.nz + iz;
}

// count: cell and in-cell slot of every point (an atomic per point: the slot order is arbitrary)
__global__ __launch_bounds__(RC_THREADS) void nn_count_kernel(const float* __restrict__ pts, int64_t n, const NnDev g,
                                                              int32_t* __restrict__ counts, int32_t* __restrict__ cell,
                                                              int32_t* __restrict__ slot) {
    const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += stride) {
        const int c = nn_cell_of(g, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        cell[i] = c;
        slot[i] = atomicAdd(&counts[c], 1);
    }
}

__global__ __launch_bounds__(RC_THREADS) void nn_scatter_ref_kernel(const float* __restrict__ pts, int64_t n,
                                                                    const int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ cell,
                                                                    const int32_t* __restrict__ slot,
                                                                    float4* __restrict__ sorted) {
    const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += stride) {
        const int64_t pos = (int64_t)start[cell[i]] + slot[i];
        sorted[pos] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i));
    }
}

__global__ __launch_bounds__(RC_THREADS) void nn_scatter_query_kernel(int64_t n, const int32_t* __restrict__ start,
                                                                      const int32_t* __restrict__ cell,
                                                                      const int32_t* __restrict__ slot,
                                                                      int32_t* __restrict__ order) {
    const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += stride)
        order[(int64_t)start[cell[i]] + slot[i]] = (int32_t)i;
}

// distance from q to the slab [lo, lo + cell] along one axis, less the slack (never negative)
__device__ __forceinline__ float nn_gap(float q, float lo, float cell, float slack) {
    return fmaxf(fmaxf(lo - q, q - (lo + cell)) - slack, 0.0f);
}

// One query per lane, in cell order when `order` is given.  Ring r = the cells at Chebyshev distance r from the query's
// clamped cell (within the grid).  After ring r every point outside the searched box B_r lies, along some axis, beyond
// one of B_r's faces that still has cells behind it, so its distance is at least the smallest such face distance (less
// a slack for the float32 rounding of the cell assignment).  The search stops when that bound squared reaches the
// best squared distance, or when B_r covers the grid.  Cells whose own box is already too far are skipped.
// best: (d2, index) minimised lexicographically, so equal distances go to the smaller reference index.
__global__ __launch_bounds__(RC_THREADS) void nn_query_kernel(const float* __restrict__ qs, int64_t nq,
                                                              const int32_t* __restrict__ order, const NnDev g,
                                                              const int32_t* __restrict__ start,
                                                              const float4* __restrict__ ref, float limit2, float max_dist,
                                                              float* __restrict__ dist, int32_t* __restrict__ idx) {
    const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; t < nq; t += stride) {
        const int64_t qi = order ? (int64_t)order[t] : t;
        const float qx = qs[3 * qi], qy = qs[3 * qi + 1], qz = qs[3 * qi + 2];
        const int cx = nn_axis_cell(qx, g.lox, g.inv, g.nx), cy = nn_axis_cell(qy, g.loy, g.inv, g.ny);
        const int cz = nn_axis_cell(qz, g.loz, g.inv, g.nz);
        const float hix = g.lox + g.nx * g.cell, hiy = g.loy + g.ny * g.cell, hiz = g.loz + g.nz * g.cell;
        const float mag = fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)) +
                          fmaxf(fmaxf(fmaxf(fabsf(g.lox), fabsf(hix)), fmaxf(fabsf(g.loy), fabsf(hiy))),
                                fmaxf(fabsf(g.loz), fabsf(hiz)));
        const float slack = 1e-6f * mag;
        float best = limit2;
        int bi = -1;
        for (int r = 0;; ++r) {
            const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r, z0 = cz - r, z1 = cz + r;
            const int zlo = max(z0, 0), zhi = min(z1, g.nz - 1);
            for (int ix = max(x0, 0); ix <= min(x1, g.nx - 1); ++ix) {
                const bool xe = ix == x0 || ix == x1;
                const float gx = nn_gap(qx, g.lox + ix * g.cell, g.cell, slack);
                for (int iy = max(y0, 0); iy <= min(y1, g.ny - 1); ++iy) {
                    const bool ye = iy == y0 || iy == y1;
                    const float gy = nn_gap(qy, g.loy + iy * g.cell, g.cell, slack);
                    const float gxy = gx * gx + gy * gy;
                    if (gxy >= best) continue;
                    const int step = (xe || ye) ? 1 : max(z1 - z0, 1);   // inner cells: only the two z faces
                    for (int iz = (xe || ye) ? zlo : z0; iz <= zhi; iz += step) {
                        if (iz < 0) continue;
                        const float gz = nn_gap(qz, g.loz + iz * g.cell, g.cell, slack);
                        if (gxy + gz * gz >= best) continue;
                        const int c = (ix * g.ny + iy) * g.nz + iz;
                        const int j1 = start[c + 1];
                        for (int j = start[c]; j < j1; ++j) {
                            const float4 p = ref[j];
                            const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
                            const float d2 = dx * dx + dy * dy + dz * dz;
                            const int pi = __float_as_int(p.w);
                            if (d2 < best || (d2 == best && pi < bi)) {
                                best = d2;
                                bi = pi;
                            }
                        }
                    }
                }
            }
            float lb = INFINITY;
            if (x0 > 0) lb = fminf(lb, qx - (g.lox + x0 * g.cell));
            if (x1 < g.nx - 1) lb = fminf(lb, (g.lox + (x1 + 1) * g.cell) - qx);
            if (y0 > 0) lb = fminf(lb, qy - (g.loy + y0 * g.cell));
            if (y1 < g.ny - 1) lb = fminf(lb, (g.loy + (y1 + 1) * g.cell) - qy);
            if (z0 > 0) lb = fminf(lb, qz - (g.loz + z0 * g.cell));
            if (z1 < g.nz - 1) lb = fminf(lb, (g.loz + (z1 + 1) * g.cell) - qz);
            if (lb == INFINITY) break;                                 // the box covers the grid
            lb -= slack;
            if (lb > 0.0f && lb * lb >= best) break;
        }
        float d = INFINITY;
        if (bi >= 0) {
            d = sqrtf(best);
            if (!(d < max_dist)) {                                     // max_dist = inf: every finite distance passes
                d = INFINITY;
                bi = -1;
            }
        }
        dist[qi] = d;
        idx[qi] = bi;
    }
}

// ---------------------------------------------------------------------------------------------------------
// ICP moments: a fixed-order float64 reduction (no float atomics)
// ---------------------------------------------------------------------------------------------------------
#define ICP_N 17

// 256 values per moment in LDS -> lds[k][0], by a fixed tree
__device__ __forceinline__ void icp_tree(double (*lds)[RC_THREADS]) {
    for (int s = RC_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < ICP_N; ++k) lds[k][threadIdx.x] += lds[k][threadIdx.x + s];
        __syncthreads();
    }
}

// workgroup b takes the correspondences [b per_block, (b + 1) per_block), thread t every 256th of them from t
__global__ __launch_bounds__(RC_THREADS) void icp_moments_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                 const float* __restrict__ dist, const int32_t* __restrict__ idx,
                                                                 int64_t n, float threshold, int64_t per_block,
                                                                 double* __restrict__ partial) {
    __shared__ double lds[ICP_N][RC_THREADS];
    double acc[ICP_N];
#pragma unroll
    for (int k = 0; k < ICP_N; ++k) acc[k] = 0.0;
    const int64_t b0 = (int64_t)blockIdx.x * per_block;
    const int64_t b1 = min(b0 + per_block, n);
    for (int64_t i = b0 + threadIdx.x; i < b1; i += RC_THREADS) {
        const int j = idx[i];
        const float d = dist[i];
        if (j < 0 || !(d < threshold)) continue;
        const double s[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
        const double t[3] = {tgt[3 * (int64_t)j], tgt[3 * (int64_t)j + 1], tgt[3 * (int64_t)j + 2]};
        acc[0] += 1.0;
        acc[1] += (double)d * (double)d;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[2 + a] += s[a];
            acc[5 + a] += t[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[8 + 3 * a + c] += s[a] * t[c];
        }
    }
#pragma unroll
    for (int k = 0; k < ICP_N; ++k) lds[k][threadIdx.x] = acc[k];
    __syncthreads();
    icp_tree(lds);
    if (threadIdx.x < ICP_N) partial[(int64_t)blockIdx.x * ICP_N + threadIdx.x] = lds[threadIdx.x][0];
}

__global__ __launch_bounds__(RC_THREADS) void icp_final_kernel(const double* __restrict__ partial, int nb,
                                                               double* __restrict__ out) {
    __shared__ double lds[ICP_N][RC_THREADS];
    for (int k = 0; k < ICP_N; ++k) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += RC_THREADS) a += partial[(int64_t)b * ICP_N + k];
        lds[k][threadIdx.x] = a;
    }
    __syncthreads();
    icp_tree(lds);
    if (threadIdx.x < ICP_N) out[threadIdx.x] = lds[threadIdx.x][0];
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static int64_t rc_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

extern "C" int eslam_cull_vertices(const float* verts, int64_t n_verts, const float* depths, int n_frames, int depth_h,
                                   int depth_w, const float* w2c, float fx, float fy, float cx, float cy, int H, int W,
                                   float truncation, int depth_test, uint8_t* seen, eslam_stream_t stream) {
    if (n_verts < 0 || n_frames < 0 || (depth_test && (depth_h < 1 || depth_w < 1))) {
        eslam_set_error("eslam_cull_vertices: bad sizes (%lld vertices, %d frames, depth %d x %d)", (long long)n_verts,
                        n_frames, depth_h, depth_w);
        return 1;
    }
    if (n_verts == 0 || n_frames == 0) return 0;
    if (!verts || !w2c || !seen || (depth_test && !depths)) {
        eslam_set_error("eslam_cull_vertices: null argument");
        return 1;
    }
    CullCam cam;
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.H = (float)H; cam.W = (float)W;
    cam.truncation = truncation; cam.depth_test = depth_test ? 1 : 0;
    hipLaunchKernelGGL(cull_vertices_kernel, dim3(rc_blocks(n_verts)), dim3(RC_THREADS), 0, (hipStream_t)stream, verts,
                       n_verts, depth_test ? depths : nullptr, n_frames, depth_h, depth_w, w2c, cam, seen);
    return eslam_check_launch("cull_vertices_kernel");
}

static bool nn_grid_ok(const char* who, const eslam_nn_grid_t* g) {
    if (!g) {
        eslam_set_error("%s: null grid", who);
        return false;
    }
    const double cells = (double)g->dims[0] * g->dims[1] * g->dims[2];
    if (g->dims[0] < 1 || g->dims[1] < 1 || g->dims[2] < 1 || cells > ESLAM_NN_MAX_CELLS || !(g->cell > 0.0f) ||
        !isfinite(g->cell) || !isfinite(g->lo[0]) || !isfinite(g->lo[1]) || !isfinite(g->lo[2])) {
        eslam_set_error("%s: invalid grid (%d x %d x %d cells of %g)", who, g->dims[0], g->dims[1], g->dims[2],
                        (double)g->cell);
        return false;
    }
    return true;
}

static int64_t nn_cells(const eslam_nn_grid_t* g) { return (int64_t)g->dims[0] * g->dims[1] * g->dims[2]; }

static NnDev nn_dev(const eslam_nn_grid_t* g) {
    NnDev d;
    d.lox = g->lo[0]; d.loy = g->lo[1]; d.loz = g->lo[2];
    d.cell = g->cell; d.inv = 1.0f / g->cell;
    d.nx = g->dims[0]; d.ny = g->dims[1]; d.nz = g->dims[2];
    return d;
}

extern "C" int eslam_nn_grid_plan(int64_t n_ref, const float* bbox6_host, eslam_nn_grid_t* grid) {
    if (n_ref < 1 || n_ref > INT32_MAX || !bbox6_host || !grid) {
        eslam_set_error("eslam_nn_grid_plan: %lld points (1 .. 2^31 - 1) or a null argument", (long long)n_ref);
        return 1;
    }
    double ext[3], E = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double lo = bbox6_host[2 * d], hi = bbox6_host[2 * d + 1];
        if (!isfinite(lo) || !isfinite(hi) || hi < lo) {
            eslam_set_error("eslam_nn_grid_plan: bad bounding box on axis %d: [%g, %g]", d, lo, hi);
            return 1;
        }
        ext[d] = hi - lo;
        E = fmax(E, ext[d]);
        grid->lo[d] = bbox6_host[2 * d];
    }
    grid->reserved = 0;
    if (!(E > 0.0)) {                                   // one point, or all points equal
        grid->cell = 1.0f;
        grid->dims[0] = grid->dims[1] = grid->dims[2] = 1;
        return 0;
    }
    int m = 0;
    double vol = 1.0;
    for (int d = 0; d < 3; ++d)
        if (ext[d] > 1e-6 * E) {                        // flat axes (extent <= 1e-6 of the largest) get one cell
            ++m;
            vol *= ext[d];
        }
    const double target = fmin((double)ESLAM_NN_MAX_CELLS, fmax(1.0, ESLAM_NN_CELLS_PER_POINT * (double)n_ref));
    double cell = pow(vol / target, 1.0 / m);
    for (;;) {
        const float cf = nextafterf((float)cell, INFINITY);     // dims * cf covers the extent
        double prod = 1.0;
        int dims[3];
        for (int d = 0; d < 3; ++d) {
            const double n = fmax(1.0, ceil(ext[d] / (double)cf));
            prod *= n;
            dims[d] = n > ESLAM_NN_MAX_CELLS ? ESLAM_NN_MAX_CELLS + 1 : (int)n;
        }
        if (prod <= ESLAM_NN_MAX_CELLS) {
            grid->cell = cf;
            for (int d = 0; d < 3; ++d) grid->dims[d] = dims[d];
            return 0;
        }
        cell *= 1.1;
    }
}

struct NnWork {
    int32_t* start;      // [cells + 1]
    int32_t* partial;    // [chunks(cells)]
    int32_t* cell;       // [n]
    int32_t* slot;       // [n]
    float4* sorted;      // [n]   (build) / int32 order [n] (query)
};

static int64_t nn_work_layout(int64_t cells, int64_t n, int elem, void* base, NnWork* w) {
    char* p = (char*)base;
    int64_t off = 0;
    if (w) w->start = (int32_t*)(p + off);
    off += rc_align(4 * (cells + 1));
    if (w) w->partial = (int32_t*)(p + off);
    off += rc_align(4 * rc_chunks(cells + 1));
    if (w) w->cell = (int32_t*)(p + off);
    off += rc_align(4 * n);
    if (w) w->slot = (int32_t*)(p + off);
    off += rc_align(4 * n);
    if (w) w->sorted = (float4*)(p + off);
    off += rc_align((int64_t)elem * n);
    return off;
}

extern "C" int64_t eslam_nn_workspace_bytes(const eslam_nn_grid_t* grid, int64_t n_ref) {
    if (!grid || n_ref < 1 || n_ref > INT32_MAX || !nn_grid_ok("eslam_nn_workspace_bytes", grid)) return -1;
    return nn_work_layout(nn_cells(grid), n_ref, 16, nullptr, nullptr);
}

extern "C" int64_t eslam_nn_query_workspace_bytes(const eslam_nn_grid_t* grid, int64_t n_query) {
    if (!grid || n_query < 0 || n_query > INT32_MAX || !nn_grid_ok("eslam_nn_query_workspace_bytes", grid)) return -1;
    return nn_work_layout(nn_cells(grid), n_query, 4, nullptr, nullptr);
}

// counting sort of n points into the grid's cells: start [cells + 1] (exclusive offsets, total at the end), cell, slot
static int nn_sort(const float* pts, int64_t n, const NnDev& g, int64_t cells, const NnWork& w, hipStream_t st) {
    if (hipMemsetAsync(w.start, 0, (size_t)(cells + 1) * 4, st) != hipSuccess) {
        eslam_set_error("nn: memset failed");
        return 2;
    }
    if (n > 0) {
        hipLaunchKernelGGL(nn_count_kernel, dim3(rc_blocks(n)), dim3(RC_THREADS), 0, st, pts, n, g, w.start, w.cell, w.slot);
        if (eslam_check_launch("nn_count_kernel")) return 1;
    }
    return rc_scan(w.start, cells, w.partial, st);
}

extern "C" int eslam_nn_build(const float* ref, int64_t n_ref, const eslam_nn_grid_t* grid, void* workspace,
                              eslam_stream_t stream) {
    if (!nn_grid_ok("eslam_nn_build", grid)) return 1;
    if (n_ref < 1 || n_ref > INT32_MAX || !ref || !workspace) {
        eslam_set_error("eslam_nn_build: %lld points (1 .. 2^31 - 1) or a null argument", (long long)n_ref);
        return 1;
    }
    const NnDev g = nn_dev(grid);
    const int64_t cells = nn_cells(grid);
    NnWork w;
    nn_work_layout(cells, n_ref, 16, workspace, &w);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = nn_sort(ref, n_ref, g, cells, w, st)) return rc;
    hipLaunchKernelGGL(nn_scatter_ref_kernel, dim3(rc_blocks(n_ref)), dim3(RC_THREADS), 0, st, ref, n_ref, w.start, w.cell,
                       w.slot, w.sorted);
    return eslam_check_launch("nn_scatter_ref_kernel");
}

extern "C" int eslam_nn_query(const eslam_nn_grid_t* grid, const void* workspace, int64_t n_ref, const float* queries,
                              int64_t n_query, float max_dist, int flags, void* query_workspace, float* dist,
                              int32_t* idx, eslam_stream_t stream) {
    if (!nn_grid_ok("eslam_nn_query", grid)) return 1;
    if (n_ref < 1 || n_ref > INT32_MAX || n_query < 0 || n_query > INT32_MAX) {
        eslam_set_error("eslam_nn_query: %lld reference points, %lld queries", (long long)n_ref, (long long)n_query);
        return 1;
    }
    if (n_query == 0) return 0;
    const bool input_order = flags & ESLAM_NN_INPUT_ORDER;
    if (!workspace || !queries || !dist || !idx || (!input_order && !query_workspace) || isnan(max_dist)) {
        eslam_set_error("eslam_nn_query: null argument or NaN max_dist");
        return 1;
    }
    const NnDev g = nn_dev(grid);
    const int64_t cells = nn_cells(grid);
    NnWork w;
    nn_work_layout(cells, n_ref, 16, const_cast<void*>(workspace), &w);
    hipStream_t st = (hipStream_t)stream;
    const int32_t* order = nullptr;
    if (!input_order) {
        NnWork q;
        nn_work_layout(cells, n_query, 4, query_workspace, &q);
        if (int rc = nn_sort(queries, n_query, g, cells, q, st)) return rc;
        int32_t* ord = (int32_t*)q.sorted;
        hipLaunchKernelGGL(nn_scatter_query_kernel, dim3(rc_blocks(n_query)), dim3(RC_THREADS), 0, st, n_query, q.start,
                           q.cell, q.slot, ord);
        if (eslam_check_launch("nn_scatter_query_kernel")) return 1;
        order = ord;
    }
    // candidates must have d2 < limit2; a little above max_dist^2 so that the exact test sqrt(d2) < max_dist decides
    const float limit2 = isinf(max_dist) ? INFINITY : max_dist * max_dist * (1.0f + 1e-6f);
    hipLaunchKernelGGL(nn_query_kernel, dim3(rc_blocks(n_query)), dim3(RC_THREADS), 0, st, queries, n_query, order, g,
                       w.start, w.sorted, limit2, max_dist, dist, idx);
    return eslam_check_launch("nn_query_kernel");
}

extern "C" int64_t eslam_icp_moments_workspace_bytes(void) { return (int64_t)ICP_BLOCKS * ICP_N * 8; }

extern "C" int eslam_icp_moments(const float* src, const float* tgt, const float* dist, const int32_t* idx, int64_t n,
                                 float threshold, void* workspace, double* out, eslam_stream_t stream) {
    if (n < 0 || !workspace || !out || (n > 0 && (!src || !tgt || !dist || !idx))) {
        eslam_set_error("eslam_icp_moments: negative count or null argument");
        return 1;
    }
    const int64_t per_block = n > 0 ? (n + ICP_BLOCKS - 1) / ICP_BLOCKS : 1;
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(icp_moments_kernel, dim3(ICP_BLOCKS), dim3(RC_THREADS), 0, st, src, tgt, dist, idx, n, threshold,
                       per_block, partial);
    if (eslam_check_launch("icp_moments_kernel")) return 1;
    hipLaunchKernelGGL(icp_final_kernel, dim3(1), dim3(RC_THREADS), 0, st, partial, ICP_BLOCKS, out);
    return eslam_check_launch("icp_final_kernel");
}
