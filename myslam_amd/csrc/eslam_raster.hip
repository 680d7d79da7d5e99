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

#define RS_THREADS 256
#define RS_TILE 64                                  // a queued tile is at most RS_TILE x RS_TILE pixels: 64 rows a wave
#define RS_QUEUE_CAP (1 << 19)                      // queue entries per view (8 bytes each)
#define RS_MAX_BLOCKS 4096                          // grid-stride loops beyond this many workgroups per view
#define RS_LARGE_BLOCKS 256                         // workgroups per view of the tile launch (4 waves each)
#define RS_BOX_SLACK 0.01f                          // pixels added around a projected box: covers the projection's rounding
#define RS_CUT_SLACK 1.0f                           // the same around the box of a triangle cut at the near plane
#define RS_MAX_IMAGE 16384
#define L1_BLOCKS 64                                // partial sums per view of eslam_depth_l1 (a constant: fixed order)

struct RsCam {
    float fx, fy, cx, cy, z_near, z_far;
    int H, W;
};

struct RsTri {
    float m0x, m0y, m0z, m1x, m1y, m1z, m2x, m2y, m2z;   // E_k = m_k . d
    float nx, ny, nz, nv0;                               // z = nv0 / (n . d)
    int x0, y0, x1, y1;                                  // pixel box, inclusive, inside the image
};

struct RsPose {
    float m[12];
};

__device__ __forceinline__ RsPose rs_pose(const float* __restrict__ w2c, int view) {
    const float* m = w2c + 12 * (int64_t)view;
    RsPose p;
#pragma unroll
    for (int k = 0; k < 12; ++k) p.m[k] = m[k];
    return p;
}

// m = v_i x v_j of the edge i -> j, taken from the edge's smaller end (camera-space x, then y, then z) with the edge as the
// second factor, lo x (hi - lo), and negated when that end is v_j.  The same value as v_i x v_j without the cancellation
// of two long, nearly parallel vectors (3 m vectors 1 cm apart: 5e-3 px of edge position otherwise), and the same bits up
// to the sign for the two triangles that share the edge - E = m . d (an fmaf chain, exact under negation) then has
// opposite signs in the two, or is zero in both: no pixel falls between them.
__device__ __forceinline__ void rs_edge(const float* vi, const float* vj, float& mx, float& my, float& mz) {
    const bool fwd = vi[0] < vj[0] || (vi[0] == vj[0] && (vi[1] < vj[1] || (vi[1] == vj[1] && vi[2] <= vj[2])));
    const float lx = fwd ? vi[0] : vj[0], ly = fwd ? vi[1] : vj[1], lz = fwd ? vi[2] : vj[2];
    const float ex = (fwd ? vj[0] : vi[0]) - lx, ey = (fwd ? vj[1] : vi[1]) - ly, ez = (fwd ? vj[2] : vi[2]) - lz;
    const float x = ly * ez - lz * ey, y = lz * ex - lx * ez, z = lx * ey - ly * ex;
    mx = fwd ? x : -x;
    my = fwd ? y : -y;
    mz = fwd ? z : -z;
}

// Triangle f of the mesh in the camera frame of `pose`; false when it cannot touch a pixel: an index outside the vertex
// array, zero area, wholly nearer than z_near (behind the camera included) or beyond z_far, or a pixel box that misses the image.
__device__ __forceinline__ bool rs_setup(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                         int64_t f, const RsPose& P, const RsCam& cam, RsTri& t) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
    float v[3][3];
    const int idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float px = verts[3 * (int64_t)idx[k]], py = verts[3 * (int64_t)idx[k] + 1], pz = verts[3 * (int64_t)idx[k] + 2];
        v[k][0] = fmaf(P.m[0], px, fmaf(P.m[1], py, fmaf(P.m[2], pz, P.m[3])));
        v[k][1] = fmaf(P.m[4], px, fmaf(P.m[5], py, fmaf(P.m[6], pz, P.m[7])));
        v[k][2] = fmaf(P.m[8], px, fmaf(P.m[9], py, fmaf(P.m[10], pz, P.m[11])));
    }
    const float zmin = fminf(fminf(v[0][2], v[1][2]), v[2][2]), zmax = fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]);
    if (!(zmax >= cam.z_near) || !(zmin <= cam.z_far)) return false;
    const float ax = v[1][0] - v[0][0], ay = v[1][1] - v[0][1], az = v[1][2] - v[0][2];     // v1 - v0
    const float cx_ = v[0][0] - v[2][0], cy_ = v[0][1] - v[2][1], cz_ = v[0][2] - v[2][2];  // v0 - v2
    // n = (v1 - v0) x (v2 - v0) = a x (-c)
    t.nx = cy_ * az - cz_ * ay;
    t.ny = cz_ * ax - cx_ * az;
    t.nz = cx_ * ay - cy_ * ax;
    if (t.nx == 0.0f && t.ny == 0.0f && t.nz == 0.0f) return false;
    t.nv0 = t.nx * v[0][0] + t.ny * v[0][1] + t.nz * v[0][2];
    rs_edge(v[1], v[2], t.m0x, t.m0y, t.m0z);
    rs_edge(v[2], v[0], t.m1x, t.m1y, t.m1z);
    rs_edge(v[0], v[1], t.m2x, t.m2y, t.m2z);
    // The pixel box of the part beyond zc = z_near / 2 (the triangle cut by that plane: nothing nearer can be a hit, and the
    // projection of an edge that does not reach z = 0 is monotone along it, so the cut polygon's corners bound it).  A
    // triangle wholly beyond the near plane is not cut: its own three projections.
    const float zc = 0.5f * cam.z_near;
    float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* a = v[k];
        const float* b = v[(k + 1) % 3];
        if (a[2] >= zc) {
            const float px = cam.fx * a[0] / a[2] + cam.cx, py = cam.fy * a[1] / a[2] + cam.cy;
            xlo = fminf(xlo, px); xhi = fmaxf(xhi, px);
            ylo = fminf(ylo, py); yhi = fmaxf(yhi, py);
        }
        if ((a[2] >= zc) != (b[2] >= zc)) {
            const float s = (zc - a[2]) / (b[2] - a[2]);
            const float px = cam.fx * (a[0] + s * (b[0] - a[0])) / zc + cam.cx, py = cam.fy * (a[1] + s * (b[1] - a[1])) / zc + cam.cy;
            xlo = fminf(xlo, px); xhi = fmaxf(xhi, px);
            ylo = fminf(ylo, py); yhi = fmaxf(yhi, py);
        }
    }
    const float slack = zmin <= cam.z_near ? RS_CUT_SLACK : RS_BOX_SLACK;
    // clamped as floats first (huge or NaN projections stay in range), then to the pixel centres inside
    t.x0 = (int)ceilf(fmaxf(xlo - slack, 0.0f));
    t.x1 = (int)floorf(fminf(xhi + slack, (float)(cam.W - 1)));
    t.y0 = (int)ceilf(fmaxf(ylo - slack, 0.0f));
    t.y1 = (int)floorf(fminf(yhi + slack, (float)(cam.H - 1)));
    return t.x0 <= t.x1 && t.y0 <= t.y1;
}

// pixel (x, y) of one view's z-buffer against one triangle; 0 <= x < W, 0 <= y < H is the caller's duty
__device__ __forceinline__ void rs_pixel(const RsTri& t, const RsCam& cam, int x, int y, uint32_t* __restrict__ zbuf) {
    const float dx = ((float)x - cam.cx) / cam.fx, dy = ((float)y - cam.cy) / cam.fy;
    const float e0 = fmaf(t.m0x, dx, fmaf(t.m0y, dy, t.m0z));
    const float e1 = fmaf(t.m1x, dx, fmaf(t.m1y, dy, t.m1z));
    const float e2 = fmaf(t.m2x, dx, fmaf(t.m2y, dy, t.m2z));
    const bool in = (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
    if (!in) return;
    const float nd = fmaf(t.nx, dx, fmaf(t.ny, dy, t.nz));
    if (nd == 0.0f) return;                              // the ray lies in the triangle's plane
    const float z = t.nv0 / nd;
    if (!(z >= cam.z_near && z <= cam.z_far)) return;
    const uint32_t bits = __float_as_uint(z);
    uint32_t* p = zbuf + (int64_t)y * cam.W + x;
    // the stored value only ever falls: a stale read is merely larger, and the atomic then decides
    if (bits < *(volatile uint32_t*)p) atomicMin(p, bits);
}

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
static int64_t rs_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static int rs_blocks(int64_t n, int cap) {
    const int64_t b = (n + RS_THREADS - 1) / RS_THREADS;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

static bool rs_sizes_ok(int64_t n_faces, int n_views, int H, int W) {
    return n_faces >= 0 && n_faces <= INT32_MAX && n_views >= 0 && H >= 1 && W >= 1 && H <= RS_MAX_IMAGE && W <= RS_MAX_IMAGE;
}

// queue entries per view: every triangle cut into all of the image's tiles, at most RS_QUEUE_CAP
static int64_t rs_queue_cap(int64_t n_faces, int H, int W) {
    const int64_t full = (int64_t)((W + RS_TILE - 1) / RS_TILE) * ((H + RS_TILE - 1) / RS_TILE);
    const int64_t want = n_faces > RS_QUEUE_CAP ? RS_QUEUE_CAP : n_faces * full;
    return want < 1 ? 1 : want > RS_QUEUE_CAP ? RS_QUEUE_CAP : want;
}

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
