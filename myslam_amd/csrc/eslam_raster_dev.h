// The depth rasteriser's device and host helpers (triangle setup, pixel box, edge functions, the pixel test and the launch
// sizes), shared by eslam_raster.hip and eslam_viewer.hip: both rasterise with the same arithmetic, bit for bit.
#pragma once
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

// The ray of pixel (x, y) against one triangle: false when it misses; else the edge functions and the depth of the hit.
__device__ __forceinline__ bool rs_hit(const RsTri& t, const RsCam& cam, int x, int y, float& e0, float& e1, float& e2, float& z) {
    const float dx = ((float)x - cam.cx) / cam.fx, dy = ((float)y - cam.cy) / cam.fy;
    e0 = fmaf(t.m0x, dx, fmaf(t.m0y, dy, t.m0z));
    e1 = fmaf(t.m1x, dx, fmaf(t.m1y, dy, t.m1z));
    e2 = fmaf(t.m2x, dx, fmaf(t.m2y, dy, t.m2z));
    const bool in = (e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f) || (e0 <= 0.0f && e1 <= 0.0f && e2 <= 0.0f);
    if (!in) return false;
    const float nd = fmaf(t.nx, dx, fmaf(t.ny, dy, t.nz));
    if (nd == 0.0f) return false;                        // the ray lies in the triangle's plane
    z = t.nv0 / nd;
    return z >= cam.z_near && z <= cam.z_far;
}

// pixel (x, y) of one view's z-buffer against one triangle; 0 <= x < W, 0 <= y < H is the caller's duty
__device__ __forceinline__ void rs_pixel(const RsTri& t, const RsCam& cam, int x, int y, uint32_t* __restrict__ zbuf) {
    float e0, e1, e2, z;
    if (!rs_hit(t, cam, x, y, e0, e1, e2, z)) return;
    const uint32_t bits = __float_as_uint(z);
    uint32_t* p = zbuf + (int64_t)y * cam.W + x;
    // the stored value only ever falls: a stale read is merely larger, and the atomic then decides
    if (bits < *(volatile uint32_t*)p) atomicMin(p, bits);
}

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
