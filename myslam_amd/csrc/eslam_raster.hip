// Depth rasteriser for triangle meshes and the 2D reconstruction metric's reductions: replaces open3d's OpenGL
// visualiser in reference src/tools/eval_recon.py:127-207 (capture_depth_float_buffer of the ground-truth mesh and of
// the reconstruction from 1000 random views), the mean absolute difference of the two images, and check_proj
// (eval_recon.py:59-85) for a batch of candidate views.
//
//   raster   one call renders a chunk of views.  The output image doubles as the z-buffer: uint32 holding the float's
//            bits (positive floats order as their bit patterns), cleared to +inf, resolved with atomicMin - order
//            independent, so two runs are bit-identical - and a last pass turns untouched pixels into 0.
//            Coverage and depth come from camera-space vertices without a perspective divide (no near-plane clipping):
//            the edge functions E_k = d . (v_i x v_j) of the pixel ray d, depth z = (n . v0) / (n . d).
//            Two triangle sizes: a 1 cm mesh seen from inside a room has triangles of about a pixel, a ground-truth room
//            has triangles that cover the image.  One lane per triangle (grid: triangle chunks x views, the view
//            wave-uniform so the pose is read with scalar loads); a triangle whose pixel box is at most `large_area`
//            pixels is rasterised by its lane, a larger one is cut into RS_TILE x RS_TILE pixel tiles that are appended
//            to the view's queue (one wave-aggregated vector atomic add per wave) and rasterised, a wave per tile, by a
//            second launch.
//   l1       per view, sum |a - b| over the pixels in float64 by a fixed-order tree (no float atomics).
//   see      one lane per point, a loop over the views, a wave vote, one vector store per wave and seeing view.
#include <math.h>

#include "eslam_common.h"
#include "eslam_raster_dev.h"

#define L1_BLOCKS 64                                // partial sums per view of eslam_depth_l1 (a constant: fixed order)

__global__ __launch_bounds__(RS_THREADS) void raster_clear_kernel(uint32_t* __restrict__ zbuf, int64_t n,
                                                                  unsigned long long* __restrict__ counters, int n_views) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    const int64_t i0 = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i0 < n_views) counters[i0] = 0ull;
    for (int64_t i = i0; i < n; i += stride) zbuf[i] = 0x7f800000u;
}

__global__ __launch_bounds__(RS_THREADS) void raster_resolve_kernel(uint32_t* __restrict__ zbuf, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += stride)
        if (zbuf[i] == 0x7f800000u) zbuf[i] = 0u;
}

// One triangle per lane.  The loop's trip count is the same for every lane of a wave (the wave's base index decides), so
// the wave-wide scan below runs with all 64 lanes active.
__global__ __launch_bounds__(RS_THREADS) void raster_small_kernel(const float* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ faces, int64_t F,
                                                                  const float* __restrict__ w2c, const RsCam cam, int large_area,
                                                                  uint32_t* __restrict__ zbuf_all,
                                                                  unsigned long long* __restrict__ counters,
                                                                  uint2* __restrict__ queue_all, int64_t cap) {
    const int view = blockIdx.y;
    const RsPose P = rs_pose(w2c, view);
    uint32_t* zbuf = zbuf_all + (int64_t)view * cam.H * cam.W;
    uint2* queue = queue_all + (int64_t)view * cap;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * RS_THREADS + (threadIdx.x & ~63); base < F; base += stride) {
        const int64_t f = base + lane;
        RsTri t;
        const bool live = f < F && rs_setup(verts, V, faces, f, P, cam, t);
        int bw = 0, bh = 0;
        if (live) {
            bw = t.x1 - t.x0 + 1;
            bh = t.y1 - t.y0 + 1;
        }
        const bool big = live && bw * bh > large_area;
        const unsigned tiles = big ? (unsigned)(((bw + RS_TILE - 1) / RS_TILE) * ((bh + RS_TILE - 1) / RS_TILE)) : 0u;
        const unsigned incl = wave_incl_sum_u(tiles);
        const unsigned total = (unsigned)__builtin_amdgcn_readlane((int)incl, WAVE - 1);
        bool own = live && !big;
        if (total) {                                      // (uniform over the wave)
            unsigned long long s = 0ull;
            if (lane == 0) s = atomicAdd(counters + view, (unsigned long long)total);
            s = __shfl(s, 0, WAVE);
            if (big) {
                const unsigned long long slot = s + (incl - tiles);
                for (unsigned k = 0; k < tiles; ++k)
                    if (slot + k < (unsigned long long)cap) queue[slot + k] = make_uint2((unsigned)f, k);
                if (slot + tiles > (unsigned long long)cap) own = true;    // what the queue cannot hold, the lane renders itself
            }
        }
        if (own)
            for (int y = t.y0; y <= t.y1; ++y)
                for (int x = t.x0; x <= t.x1; ++x) rs_pixel(t, cam, x, y, zbuf);
    }
}

// One queued tile per wave: its lanes cover 64 / (tile width) rows at a time.
__global__ __launch_bounds__(RS_THREADS) void raster_large_kernel(const float* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ faces,
                                                                  const float* __restrict__ w2c, const RsCam cam,
                                                                  uint32_t* __restrict__ zbuf_all,
                                                                  const unsigned long long* __restrict__ counters,
                                                                  const uint2* __restrict__ queue_all, int64_t cap) {
    const int view = blockIdx.y;
    const unsigned long long pushed = counters[view];
    const int64_t count = pushed < (unsigned long long)cap ? (int64_t)pushed : cap;
    const int wave = blockIdx.x * (RS_THREADS / WAVE) + (threadIdx.x >> 6), nwaves = gridDim.x * (RS_THREADS / WAVE);
    if (wave >= count) return;
    const RsPose P = rs_pose(w2c, view);
    uint32_t* zbuf = zbuf_all + (int64_t)view * cam.H * cam.W;
    const uint2* queue = queue_all + (int64_t)view * cap;
    const int lane = threadIdx.x & 63;
    for (int64_t q = wave; q < count; q += nwaves) {
        const uint2 e = queue[q];
        const int64_t f = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)e.x);
        const int tile = __builtin_amdgcn_readfirstlane((int)e.y);
        RsTri t;
        if (!rs_setup(verts, V, faces, f, P, cam, t)) continue;     // (cannot happen: the same arithmetic queued it)
        const int tiles_x = (t.x1 - t.x0 + RS_TILE) / RS_TILE;
        const int tx0 = t.x0 + RS_TILE * (tile % tiles_x), ty0 = t.y0 + RS_TILE * (tile / tiles_x);
        const int tx1 = min(tx0 + RS_TILE - 1, t.x1), ty1 = min(ty0 + RS_TILE - 1, t.y1);
        if (ty0 > t.y1) continue;
        const int tw = tx1 - tx0 + 1, rows = RS_TILE / tw;
        const int lx = lane % tw, ly = lane / tw;
        if (ly < rows)
            for (int y = ty0 + ly; y <= ty1; y += rows) rs_pixel(t, cam, tx0 + lx, y, zbuf);
    }
}

// ---------------------------------------------------------------------------------------------------------
// depth L1: per view, sum |a - b| in float64 by a fixed tree
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double l1_tree(double* lds, double v) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = RS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

// workgroup b of view k takes the pixels [b per_block, (b + 1) per_block), thread t every 256th of them from t
__global__ __launch_bounds__(RS_THREADS) void depth_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                      int64_t npix, int64_t per_block,
                                                                      double* __restrict__ partial) {
    __shared__ double lds[RS_THREADS];
    const int64_t off = (int64_t)blockIdx.y * npix;
    const int64_t b0 = (int64_t)blockIdx.x * per_block, b1 = min(b0 + per_block, npix);
    double acc = 0.0;
    for (int64_t i = b0 + threadIdx.x; i < b1; i += RS_THREADS) acc += fabs((double)a[off + i] - (double)b[off + i]);
    const double s = l1_tree(lds, acc);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * L1_BLOCKS + blockIdx.x] = s;
}

__global__ __launch_bounds__(RS_THREADS) void depth_l1_final_kernel(const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double lds[RS_THREADS];
    const double s = l1_tree(lds, threadIdx.x < L1_BLOCKS ? partial[(int64_t)blockIdx.x * L1_BLOCKS + threadIdx.x] : 0.0);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------------------
// check_proj (eval_recon.py:59-85) for a chunk of views
// ---------------------------------------------------------------------------------------------------------
// One point per lane; the trip count is uniform over the wave and k over the workgroup (scalar pose loads).  Steps, with
// w2c[k] the inverse of c2w[k] with columns 1 and 2 negated (float32 [3][4]):
//   1. c = w2c [p, 1];   2. c.x *= -1;   3. a = fx c.x + cx c.z,  b = fy c.y + cy c.z,  z = c.z + 1e-5   (K c)
//   4. u = a / z,  v = b / z;   5. the point is in view when 0 <= -z, 0 < u < W and 0 < v < H
__global__ __launch_bounds__(RS_THREADS) void views_see_points_kernel(const float* __restrict__ pts, int64_t N,
                                                                      const float* __restrict__ w2c, int K, float fx, float fy,
                                                                      float cx, float cy, float H, float W,
                                                                      uint8_t* __restrict__ seen) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * RS_THREADS + (threadIdx.x & ~63); base < N; base += stride) {
        const int64_t i = base + lane;
        const bool live = i < N;
        const float px = live ? pts[3 * i] : 0.0f, py = live ? pts[3 * i + 1] : 0.0f, pz = live ? pts[3 * i + 2] : 0.0f;
        for (int k = 0; k < K; ++k) {
            const float* m = w2c + 12 * k;
            const float cx_ = m[0] * px + m[1] * py + m[2] * pz + m[3];
            const float cy_ = m[4] * px + m[5] * py + m[6] * pz + m[7];
            const float cz_ = m[8] * px + m[9] * py + m[10] * pz + m[11];
            const float a = fx * (-cx_) + cx * cz_;
            const float b = fy * cy_ + cy * cz_;
            const float z = cz_ + 1e-5f;
            const float u = a / z, v = b / z;
            const bool ok = live && (0.0f <= -z) && (u < W) && (u > 0.0f) && (v < H) && (v > 0.0f);
            const unsigned long long vote = __ballot(ok);
            if (vote != 0ull && lane == (int)__builtin_ctzll(vote)) seen[k] = 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
extern "C" int64_t eslam_raster_workspace_bytes(int64_t n_faces, int n_views, int H, int W) {
    if (!rs_sizes_ok(n_faces, n_views, H, W)) return -1;
    return rs_align(8 * (int64_t)n_views) + 8 * rs_queue_cap(n_faces, H, W) * n_views;
}

extern "C" int eslam_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                  const float* w2c, int n_views, float fx, float fy, float cx, float cy, int H, int W,
                                  float z_near, float z_far, int large_area, void* workspace, float* depth,
                                  eslam_stream_t stream) {
    if (!rs_sizes_ok(n_faces, n_views, H, W) || n_verts < 0 || n_verts > INT32_MAX) {
        eslam_set_error("eslam_raster_depth: bad sizes (%lld vertices, %lld faces, %d views, image %d x %d; at most %d a side)",
                        (long long)n_verts, (long long)n_faces, n_views, H, W, RS_MAX_IMAGE);
        return 1;
    }
    if (!(z_near > 0.0f) || !(z_far >= z_near) || !isfinite(z_far) || !(fx != 0.0f) || !(fy != 0.0f) || !isfinite(fx) ||
        !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) {
        eslam_set_error("eslam_raster_depth: needs 0 < z_near <= z_far < inf and finite intrinsics with fx, fy != 0");
        return 1;
    }
    if (n_views == 0) return 0;
    if (!w2c || !depth || !workspace || (n_faces > 0 && (!verts || !faces))) {
        eslam_set_error("eslam_raster_depth: null argument");
        return 1;
    }
    RsCam cam;
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.z_near = z_near; cam.z_far = z_far; cam.H = H; cam.W = W;
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)n_views * H * W;
    const int64_t cap = rs_queue_cap(n_faces, H, W);
    unsigned long long* counters = (unsigned long long*)workspace;
    uint2* queue = (uint2*)((char*)workspace + rs_align(8 * (int64_t)n_views));
    uint32_t* zbuf = (uint32_t*)depth;
    hipLaunchKernelGGL(raster_clear_kernel, dim3(rs_blocks(npix, 1 << 16)), dim3(RS_THREADS), 0, st, zbuf, npix, counters,
                       n_views);
    if (eslam_check_launch("raster_clear_kernel")) return 1;
    if (n_faces > 0) {
        for (int v0 = 0; v0 < n_views; v0 += 65535) {    // (grid.y limit)
            const int nv = n_views - v0 < 65535 ? n_views - v0 : 65535;
            hipLaunchKernelGGL(raster_small_kernel, dim3(rs_blocks(n_faces, RS_MAX_BLOCKS), nv), dim3(RS_THREADS), 0, st, verts,
                               n_verts, faces, n_faces, w2c + 12 * (int64_t)v0, cam, large_area > 0 ? large_area : ESLAM_RASTER_LARGE_AREA,
                               zbuf + (int64_t)v0 * H * W, counters + v0, queue + (int64_t)v0 * cap, cap);
            if (eslam_check_launch("raster_small_kernel")) return 1;
            hipLaunchKernelGGL(raster_large_kernel, dim3(RS_LARGE_BLOCKS, nv), dim3(RS_THREADS), 0, st, verts, n_verts, faces,
                               w2c + 12 * (int64_t)v0, cam, zbuf + (int64_t)v0 * H * W, counters + v0, queue + (int64_t)v0 * cap, cap);
            if (eslam_check_launch("raster_large_kernel")) return 1;
        }
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(rs_blocks(npix, 1 << 16)), dim3(RS_THREADS), 0, st, zbuf, npix);
    return eslam_check_launch("raster_resolve_kernel");
}

extern "C" int64_t eslam_depth_l1_workspace_bytes(int n_views) {
    return n_views < 0 ? -1 : (int64_t)(n_views < 1 ? 1 : n_views) * L1_BLOCKS * 8;
}

extern "C" int eslam_depth_l1(const float* a, const float* b, int n_views, int64_t n_pixels, void* workspace, double* out,
                              eslam_stream_t stream) {
    if (n_views < 0 || n_views > 65535 || n_pixels < 0) {
        eslam_set_error("eslam_depth_l1: bad sizes (%d views (at most 65535), %lld pixels)", n_views, (long long)n_pixels);
        return 1;
    }
    if (n_views == 0) return 0;
    if (!workspace || !out || (n_pixels > 0 && (!a || !b))) {
        eslam_set_error("eslam_depth_l1: null argument");
        return 1;
    }
    const int64_t per_block = n_pixels > 0 ? (n_pixels + L1_BLOCKS - 1) / L1_BLOCKS : 1;
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(depth_l1_partial_kernel, dim3(L1_BLOCKS, n_views), dim3(RS_THREADS), 0, st, a, b, n_pixels, per_block,
                       partial);
    if (eslam_check_launch("depth_l1_partial_kernel")) return 1;
    hipLaunchKernelGGL(depth_l1_final_kernel, dim3(n_views), dim3(RS_THREADS), 0, st, partial, out);
    return eslam_check_launch("depth_l1_final_kernel");
}

extern "C" int eslam_views_see_points(const float* points, int64_t n_points, const float* w2c, int n_views, float fx, float fy,
                                      float cx, float cy, int H, int W, uint8_t* seen, eslam_stream_t stream) {
    if (n_points < 0 || n_views < 0) {
        eslam_set_error("eslam_views_see_points: bad sizes (%lld points, %d views)", (long long)n_points, n_views);
        return 1;
    }
    if (n_points == 0 || n_views == 0) return 0;
    if (!points || !w2c || !seen) {
        eslam_set_error("eslam_views_see_points: null argument");
        return 1;
    }
    hipLaunchKernelGGL(views_see_points_kernel, dim3(rs_blocks(n_points, RS_MAX_BLOCKS)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       points, n_points, w2c, n_views, fx, fy, cx, cy, (float)H, (float)W, seen);
    return eslam_check_launch("views_see_points_kernel");
}
