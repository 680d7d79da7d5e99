// Headless colour renderer for the offline viewer: replaces the open3d window of reference src/tools/visualizer_util.py:178-200
// (an unlit mesh with back faces hidden plus point clouds drawn `size` pixels wide) for machines without a display.
//
//   keys     all geometry of a view composes through one buffer of uint64 keys, [n_views][H][W]: the high word is the bits of
//            the camera-space depth (a positive float orders as its bits), the low word the pixel's RGBA8 (R in the lowest
//            byte).  begin clears it to all ones, every fragment does a 64-bit atomicMin: the nearest fragment wins, equal
//            depths go to the smaller colour word - independent of the order of calls and launches, bit-identical run to
//            run.  The atomic is gated by a 32-bit read of the stored high word, which only ever falls.
//   mesh     the depth rasteriser's setup, pixel box, edge functions and depth (eslam_raster_dev.h) and its two triangle
//            paths; colour by the edge functions as barycentrics, b_k = E_k / (E_0 + E_1 + E_2): perspective-correct, since
//            E_0 = d . (v1 x v2) = b_0 det[v0 v1 v2] / z.
//   points   one lane per point, the view wave-uniform; a point covers size x size pixels.
//   resolve  keys -> uint8 RGB and, when asked, float32 depth; untouched pixels get the background and depth 0.
#include <math.h>

#include "eslam_common.h"
#include "eslam_raster_dev.h"

#define VW_EMPTY 0xffffffffffffffffull
#define VW_GREY 0xffc8c8c8u                         // (200, 200, 200, 255): a mesh without vertex colours
#define VW_MAX_POINT_SIZE ESLAM_VIEWER_MAX_POINT_SIZE

struct VwCol {
    uint32_t c0, c1, c2;                            // the three vertices' RGBA8 words
};

__device__ __forceinline__ void vw_put(unsigned long long* __restrict__ p, uint32_t zbits, uint32_t rgba) {
    // the stored high word only ever falls: a stale read is merely larger, and the atomic then decides (little endian: word 1)
    if (zbits > ((volatile uint32_t*)p)[1]) return;
    atomicMin(p, ((unsigned long long)zbits << 32) | rgba);
}

__device__ __forceinline__ float vw_channel(uint32_t c0, uint32_t c1, uint32_t c2, int shift, float b0, float b1, float b2) {
    const float a0 = (float)((c0 >> shift) & 255u), a1 = (float)((c1 >> shift) & 255u), a2 = (float)((c2 >> shift) & 255u);
    const float c = fminf(fmaxf(b0 * a0 + b1 * a1 + b2 * a2, 0.0f), 255.0f);
    return floorf(c + 0.5f);
}

// pixel (x, y) of one view's keys against one triangle; 0 <= x < W, 0 <= y < H is the caller's duty
__device__ __forceinline__ void vw_pixel(const RsTri& t, const VwCol& col, const RsCam& cam, int x, int y,
                                         unsigned long long* __restrict__ keys) {
    float e0, e1, e2, z;
    if (!rs_hit(t, cam, x, y, e0, e1, e2, z)) return;
    const float s = e0 + e1 + e2;
    float b0 = 1.0f, b1 = 0.0f, b2 = 0.0f;          // (s = 0 with a hit: the triangle is seen edge-on; vertex 0's colour)
    if (s != 0.0f) {
        b0 = e0 / s;
        b1 = e1 / s;
        b2 = e2 / s;
    }
    const uint32_t r = (uint32_t)vw_channel(col.c0, col.c1, col.c2, 0, b0, b1, b2);
    const uint32_t g = (uint32_t)vw_channel(col.c0, col.c1, col.c2, 8, b0, b1, b2);
    const uint32_t b = (uint32_t)vw_channel(col.c0, col.c1, col.c2, 16, b0, b1, b2);
    vw_put(keys + (int64_t)y * cam.W + x, __float_as_uint(z), r | (g << 8) | (b << 16) | 0xff000000u);
}

// the colours of triangle f's vertices (rs_setup has checked its indices)
__device__ __forceinline__ VwCol vw_colors(const uint32_t* __restrict__ colors, const int32_t* __restrict__ faces, int64_t f) {
    VwCol c;
    c.c0 = c.c1 = c.c2 = VW_GREY;
    if (colors) {
        c.c0 = colors[faces[3 * f]];
        c.c1 = colors[faces[3 * f + 1]];
        c.c2 = colors[faces[3 * f + 2]];
    }
    return c;
}

__global__ __launch_bounds__(RS_THREADS) void viewer_clear_kernel(unsigned long long* __restrict__ keys, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += stride) keys[i] = VW_EMPTY;
}

__global__ __launch_bounds__(RS_THREADS) void viewer_counters_kernel(unsigned long long* __restrict__ counters, int n_views) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i < n_views) counters[i] = 0ull;
}

// One triangle per lane, as raster_small_kernel: the trip count is uniform over a wave, so the scan runs with 64 lanes.
__global__ __launch_bounds__(RS_THREADS) void viewer_small_kernel(const float* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ faces, int64_t F,
                                                                  const uint32_t* __restrict__ colors,
                                                                  const float* __restrict__ w2c, const RsCam cam, int cull,
                                                                  int large_area, unsigned long long* __restrict__ keys_all,
                                                                  unsigned long long* __restrict__ counters,
                                                                  uint2* __restrict__ queue_all, int64_t cap) {
    const int view = blockIdx.y;
    const RsPose P = rs_pose(w2c, view);
    unsigned long long* keys = keys_all + (int64_t)view * cam.H * cam.W;
    uint2* queue = queue_all + (int64_t)view * cap;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * RS_THREADS + (threadIdx.x & ~63); base < F; base += stride) {
        const int64_t f = base + lane;
        RsTri t;
        bool live = f < F && rs_setup(verts, V, faces, f, P, cam, t);
        if (live && cull && t.nv0 >= 0.0f) live = false;  // (v1 - v0) x (v2 - v0) points away from the camera: a back face
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
        if (own) {
            const VwCol col = vw_colors(colors, faces, f);
            for (int y = t.y0; y <= t.y1; ++y)
                for (int x = t.x0; x <= t.x1; ++x) vw_pixel(t, col, cam, x, y, keys);
        }
    }
}

// One queued tile per wave, as raster_large_kernel.  A queued triangle has passed the back-face rule already.
__global__ __launch_bounds__(RS_THREADS) void viewer_large_kernel(const float* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ faces,
                                                                  const uint32_t* __restrict__ colors,
                                                                  const float* __restrict__ w2c, const RsCam cam,
                                                                  unsigned long long* __restrict__ keys_all,
                                                                  const unsigned long long* __restrict__ counters,
                                                                  const uint2* __restrict__ queue_all, int64_t cap) {
    const int view = blockIdx.y;
    const unsigned long long pushed = counters[view];
    const int64_t count = pushed < (unsigned long long)cap ? (int64_t)pushed : cap;
    const int wave = blockIdx.x * (RS_THREADS / WAVE) + (threadIdx.x >> 6), nwaves = gridDim.x * (RS_THREADS / WAVE);
    if (wave >= count) return;
    const RsPose P = rs_pose(w2c, view);
    unsigned long long* keys = keys_all + (int64_t)view * cam.H * cam.W;
    const uint2* queue = queue_all + (int64_t)view * cap;
    const int lane = threadIdx.x & 63;
    for (int64_t q = wave; q < count; q += nwaves) {
        const uint2 e = queue[q];
        const int64_t f = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)e.x);
        const int tile = __builtin_amdgcn_readfirstlane((int)e.y);
        RsTri t;
        if (!rs_setup(verts, V, faces, f, P, cam, t)) continue;     // (cannot happen: the same arithmetic queued it)
        const VwCol col = vw_colors(colors, faces, f);
        const int tiles_x = (t.x1 - t.x0 + RS_TILE) / RS_TILE;
        const int tx0 = t.x0 + RS_TILE * (tile % tiles_x), ty0 = t.y0 + RS_TILE * (tile / tiles_x);
        const int tx1 = min(tx0 + RS_TILE - 1, t.x1), ty1 = min(ty0 + RS_TILE - 1, t.y1);
        if (ty0 > t.y1) continue;
        const int tw = tx1 - tx0 + 1, rows = RS_TILE / tw;
        const int lx = lane % tw, ly = lane / tw;
        if (ly < rows)
            for (int y = ty0 + ly; y <= ty1; y += rows) vw_pixel(t, col, cam, tx0 + lx, y, keys);
    }
}

// One point per lane, the view uniform over the workgroup (scalar pose loads).  Steps, float32 operation by operation:
//   1. c = w2c [p, 1], each row ((m0 px + m1 py) + m2 pz) + m3;   2. skipped unless z_near <= c.z <= z_far
//   3. u = fx c.x / c.z + cx,  v = fy c.y / c.z + cy
//   4. x0 = (int)ceil(clamp(u - size / 2, -size, W)), y0 likewise with H: the point covers x0 .. x0 + size - 1, y0 .. y0 + size - 1
__global__ __launch_bounds__(RS_THREADS) void viewer_points_kernel(const float* __restrict__ pts, int64_t N,
                                                                   const uint32_t* __restrict__ rgba, int per_point, int size,
                                                                   const float* __restrict__ w2c, const RsCam cam,
                                                                   unsigned long long* __restrict__ keys_all) {
    const int view = blockIdx.y;
    const RsPose P = rs_pose(w2c, view);
    unsigned long long* keys = keys_all + (int64_t)view * cam.H * cam.W;
    const float half = 0.5f * (float)size;
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < N; i += stride) {
        const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
        const float x = P.m[0] * px + P.m[1] * py + P.m[2] * pz + P.m[3];
        const float y = P.m[4] * px + P.m[5] * py + P.m[6] * pz + P.m[7];
        const float z = P.m[8] * px + P.m[9] * py + P.m[10] * pz + P.m[11];
        if (!(z >= cam.z_near && z <= cam.z_far)) continue;
        const float u = cam.fx * x / z + cam.cx, v = cam.fy * y / z + cam.cy;
        // clamped as floats first (huge or NaN projections stay in range)
        const int x0 = (int)ceilf(fminf(fmaxf(u - half, -(float)size), (float)cam.W));
        const int y0 = (int)ceilf(fminf(fmaxf(v - half, -(float)size), (float)cam.H));
        const int xa = max(x0, 0), xb = min(x0 + size - 1, cam.W - 1);
        const int ya = max(y0, 0), yb = min(y0 + size - 1, cam.H - 1);
        const uint32_t col = rgba[per_point ? i : 0] | 0xff000000u;
        const uint32_t zbits = __float_as_uint(z);
        for (int yy = ya; yy <= yb; ++yy)
            for (int xx = xa; xx <= xb; ++xx) vw_put(keys + (int64_t)yy * cam.W + xx, zbits, col);
    }
}

__global__ __launch_bounds__(RS_THREADS) void viewer_resolve_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                                    uint32_t background, uint8_t* __restrict__ image,
                                                                    float* __restrict__ depth) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += stride) {
        const unsigned long long k = keys[i];
        const bool hit = k != VW_EMPTY;
        const uint32_t c = hit ? (uint32_t)k : background;
        image[3 * i] = (uint8_t)(c & 255u);
        image[3 * i + 1] = (uint8_t)((c >> 8) & 255u);
        image[3 * i + 2] = (uint8_t)((c >> 16) & 255u);
        if (depth) depth[i] = hit ? __uint_as_float((uint32_t)(k >> 32)) : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side.  workspace: the keys, then the tile counters, then the tile queues
// ---------------------------------------------------------------------------------------------------------
static int64_t vw_keys_bytes(int n_views, int H, int W) { return rs_align(8 * (int64_t)n_views * H * W); }

static bool vw_camera_ok(const char* who, float fx, float fy, float cx, float cy, float z_near, float z_far) {
    if (!(z_near > 0.0f) || !(z_far >= z_near) || !isfinite(z_far) || !(fx != 0.0f) || !(fy != 0.0f) || !isfinite(fx) ||
        !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) {
        eslam_set_error("%s: needs 0 < z_near <= z_far < inf and finite intrinsics with fx, fy != 0", who);
        return false;
    }
    return true;
}

static RsCam vw_cam(float fx, float fy, float cx, float cy, int H, int W, float z_near, float z_far) {
    RsCam cam;
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy; cam.z_near = z_near; cam.z_far = z_far; cam.H = H; cam.W = W;
    return cam;
}

extern "C" int64_t eslam_viewer_workspace_bytes(int64_t n_faces, int n_views, int H, int W) {
    if (!rs_sizes_ok(n_faces, n_views, H, W)) return -1;
    return vw_keys_bytes(n_views, H, W) + rs_align(8 * (int64_t)n_views) + 8 * rs_queue_cap(n_faces, H, W) * n_views;
}

extern "C" int eslam_viewer_begin(int n_views, int H, int W, void* workspace, eslam_stream_t stream) {
    if (!rs_sizes_ok(0, n_views, H, W)) {
        eslam_set_error("eslam_viewer_begin: bad sizes (%d views, image %d x %d; at most %d a side)", n_views, H, W, RS_MAX_IMAGE);
        return 1;
    }
    if (n_views == 0) return 0;
    if (!workspace) {
        eslam_set_error("eslam_viewer_begin: null argument");
        return 1;
    }
    const int64_t npix = (int64_t)n_views * H * W;
    hipLaunchKernelGGL(viewer_clear_kernel, dim3(rs_blocks(npix, 1 << 16)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       (unsigned long long*)workspace, npix);
    return eslam_check_launch("viewer_clear_kernel");
}

extern "C" int eslam_viewer_mesh(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                 const uint8_t* colors, const float* w2c, int n_views, float fx, float fy, float cx, float cy,
                                 int H, int W, float z_near, float z_far, int cull_backfaces, int large_area, void* workspace,
                                 eslam_stream_t stream) {
    if (!rs_sizes_ok(n_faces, n_views, H, W) || n_verts < 0 || n_verts > INT32_MAX) {
        eslam_set_error("eslam_viewer_mesh: bad sizes (%lld vertices, %lld faces, %d views, image %d x %d; at most %d a side)",
                        (long long)n_verts, (long long)n_faces, n_views, H, W, RS_MAX_IMAGE);
        return 1;
    }
    if (!vw_camera_ok("eslam_viewer_mesh", fx, fy, cx, cy, z_near, z_far)) return 1;
    if (n_views == 0 || n_faces == 0) return 0;
    if (!w2c || !workspace || !verts || !faces) {
        eslam_set_error("eslam_viewer_mesh: null argument");
        return 1;
    }
    const RsCam cam = vw_cam(fx, fy, cx, cy, H, W, z_near, z_far);
    hipStream_t st = (hipStream_t)stream;
    const int64_t cap = rs_queue_cap(n_faces, H, W);
    unsigned long long* keys = (unsigned long long*)workspace;
    unsigned long long* counters = (unsigned long long*)((char*)workspace + vw_keys_bytes(n_views, H, W));
    uint2* queue = (uint2*)((char*)counters + rs_align(8 * (int64_t)n_views));
    hipLaunchKernelGGL(viewer_counters_kernel, dim3(rs_blocks(n_views, 1 << 16)), dim3(RS_THREADS), 0, st, counters, n_views);
    if (eslam_check_launch("viewer_counters_kernel")) return 1;
    for (int v0 = 0; v0 < n_views; v0 += 65535) {        // (grid.y limit)
        const int nv = n_views - v0 < 65535 ? n_views - v0 : 65535;
        hipLaunchKernelGGL(viewer_small_kernel, dim3(rs_blocks(n_faces, RS_MAX_BLOCKS), nv), dim3(RS_THREADS), 0, st, verts, n_verts,
                           faces, n_faces, (const uint32_t*)colors, w2c + 12 * (int64_t)v0, cam, cull_backfaces ? 1 : 0,
                           large_area > 0 ? large_area : ESLAM_RASTER_LARGE_AREA, keys + (int64_t)v0 * H * W, counters + v0,
                           queue + (int64_t)v0 * cap, cap);
        if (eslam_check_launch("viewer_small_kernel")) return 1;
        hipLaunchKernelGGL(viewer_large_kernel, dim3(RS_LARGE_BLOCKS, nv), dim3(RS_THREADS), 0, st, verts, n_verts, faces,
                           (const uint32_t*)colors, w2c + 12 * (int64_t)v0, cam, keys + (int64_t)v0 * H * W, counters + v0,
                           queue + (int64_t)v0 * cap, cap);
        if (eslam_check_launch("viewer_large_kernel")) return 1;
    }
    return 0;
}

extern "C" int eslam_viewer_points(const float* points, int64_t n_points, const uint8_t* rgba, int per_point, int size,
                                   const float* w2c, int n_views, float fx, float fy, float cx, float cy, int H, int W,
                                   float z_near, float z_far, void* workspace, eslam_stream_t stream) {
    if (!rs_sizes_ok(0, n_views, H, W) || n_points < 0) {
        eslam_set_error("eslam_viewer_points: bad sizes (%lld points, %d views, image %d x %d; at most %d a side)",
                        (long long)n_points, n_views, H, W, RS_MAX_IMAGE);
        return 1;
    }
    if (size < 1 || size > VW_MAX_POINT_SIZE) {
        eslam_set_error("eslam_viewer_points: point size %d outside [1, %d]", size, VW_MAX_POINT_SIZE);
        return 1;
    }
    if (!vw_camera_ok("eslam_viewer_points", fx, fy, cx, cy, z_near, z_far)) return 1;
    if (n_views == 0 || n_points == 0) return 0;
    if (!points || !rgba || !w2c || !workspace) {
        eslam_set_error("eslam_viewer_points: null argument");
        return 1;
    }
    const RsCam cam = vw_cam(fx, fy, cx, cy, H, W, z_near, z_far);
    unsigned long long* keys = (unsigned long long*)workspace;
    for (int v0 = 0; v0 < n_views; v0 += 65535) {        // (grid.y limit)
        const int nv = n_views - v0 < 65535 ? n_views - v0 : 65535;
        hipLaunchKernelGGL(viewer_points_kernel, dim3(rs_blocks(n_points, RS_MAX_BLOCKS), nv), dim3(RS_THREADS), 0,
                           (hipStream_t)stream, points, n_points, (const uint32_t*)rgba, per_point ? 1 : 0, size,
                           w2c + 12 * (int64_t)v0, cam, keys + (int64_t)v0 * H * W);
        if (eslam_check_launch("viewer_points_kernel")) return 1;
    }
    return 0;
}

extern "C" int eslam_viewer_resolve(int n_views, int H, int W, int bg_r, int bg_g, int bg_b, const void* workspace,
                                    uint8_t* image, float* depth, eslam_stream_t stream) {
    if (!rs_sizes_ok(0, n_views, H, W)) {
        eslam_set_error("eslam_viewer_resolve: bad sizes (%d views, image %d x %d; at most %d a side)", n_views, H, W, RS_MAX_IMAGE);
        return 1;
    }
    if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) {
        eslam_set_error("eslam_viewer_resolve: background (%d, %d, %d) outside [0, 255]", bg_r, bg_g, bg_b);
        return 1;
    }
    if (n_views == 0) return 0;
    if (!workspace || !image) {
        eslam_set_error("eslam_viewer_resolve: null argument");
        return 1;
    }
    const int64_t npix = (int64_t)n_views * H * W;
    const uint32_t bg = (uint32_t)bg_r | ((uint32_t)bg_g << 8) | ((uint32_t)bg_b << 16) | 0xff000000u;
    hipLaunchKernelGGL(viewer_resolve_kernel, dim3(rs_blocks(npix, 1 << 16)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       (const unsigned long long*)workspace, npix, bg, image, depth);
    return eslam_check_launch("viewer_resolve_kernel");
}

// ---------------------------------------------------------------------------------------------------------
// headlight Lambert shading of vertex colours, per view, before rasterisation (the light sits at the camera centre)
// ---------------------------------------------------------------------------------------------------------
// One vertex per lane, float32 operation by operation: l = c - v; nn = (nx nx + ny ny) + nz nz, ll likewise;
// k = 1 when nn == 0 or ll == 0, else ambient + (1 - ambient) max(0, ((nx lx + ny ly) + nz lz) / (sqrt(nn) sqrt(ll)));
// channel = (uint8)floor(min(255, c k) + 0.5), alpha 255.
__global__ __launch_bounds__(RS_THREADS) void shade_vertices_kernel(const float* __restrict__ verts, const float* __restrict__ normals,
                                                                    const uint32_t* __restrict__ rgba, int64_t V, float cx, float cy,
                                                                    float cz, float ambient, uint32_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < V; i += stride) {
        const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
        const float lx = cx - verts[3 * i], ly = cy - verts[3 * i + 1], lz = cz - verts[3 * i + 2];
        const float nn = nx * nx + ny * ny + nz * nz, ll = lx * lx + ly * ly + lz * lz;
        float k = 1.0f;
        if (nn != 0.0f && ll != 0.0f) {
            const float c = (nx * lx + ny * ly + nz * lz) / (sqrtf(nn) * sqrtf(ll));
            k = ambient + (1.0f - ambient) * fmaxf(0.0f, c);
        }
        const uint32_t col = rgba ? rgba[i] : 0x00c8c8c8u;
        uint32_t o = 0xff000000u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float c = (float)((col >> (8 * ch)) & 255u) * k;
            o |= (uint32_t)floorf(fminf(255.0f, c) + 0.5f) << (8 * ch);
        }
        out[i] = o;
    }
}

extern "C" int eslam_shade_vertices(const float* verts, const float* normals, const uint8_t* colors, int64_t n_verts,
                                    const float* cam_center3_host, float ambient, uint8_t* out, eslam_stream_t stream) {
    if (n_verts < 0 || n_verts > INT32_MAX) {
        eslam_set_error("eslam_shade_vertices: bad size (%lld vertices)", (long long)n_verts);
        return 1;
    }
    if (!(ambient >= 0.0f && ambient <= 1.0f)) {
        eslam_set_error("eslam_shade_vertices: ambient %g outside [0, 1]", (double)ambient);
        return 1;
    }
    if (!cam_center3_host) {
        eslam_set_error("eslam_shade_vertices: null argument");
        return 1;
    }
    if (!isfinite(cam_center3_host[0]) || !isfinite(cam_center3_host[1]) || !isfinite(cam_center3_host[2])) {
        eslam_set_error("eslam_shade_vertices: the camera centre is not finite");
        return 1;
    }
    if (n_verts == 0) return 0;
    if (!verts || !normals || !out) {
        eslam_set_error("eslam_shade_vertices: null argument");
        return 1;
    }
    if (((uintptr_t)out & 3) || ((uintptr_t)colors & 3)) {
        eslam_set_error("eslam_shade_vertices: colours must be 4-byte aligned");
        return 1;
    }
    hipLaunchKernelGGL(shade_vertices_kernel, dim3(rs_blocks(n_verts, RS_MAX_BLOCKS)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       verts, normals, (const uint32_t*)colors, n_verts, cam_center3_host[0], cam_center3_host[1],
                       cam_center3_host[2], ambient, (uint32_t*)out);
    return eslam_check_launch("shade_vertices_kernel");
}
