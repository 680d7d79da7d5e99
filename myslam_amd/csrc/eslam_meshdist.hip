// Exact point-to-mesh distance (include/eslam_hip.h, eslam_tri_*): a uniform grid over the mesh's bounding box, a face
// entered in every cell its axis-aligned box overlaps, and the ring search of nn_query_kernel (eslam_recon.hip) with
// triangles in place of points.
//
//   count    per face the number of cells of its box, summed in int64 (the caller sizes the workspace from it);
//   build    count per cell (an atomic per entry), exclusive scan, fill: the fill's atomic on a cell's start turns it into
//            the cell's end, so after the build cell c holds the entries [ends[c - 1], ends[c]) (ends[-1] = 0), as three
//            float4 each: (a, face), (b, 0), (c, 0);
//   query    one query per lane, in cell order by default (the counting sort of the queries below), rings of cells
//            until the distance to everything outside the searched box is at least the best so far.  A face's closest
//            point lies in the face's box, so in a cell the face is entered in: what holds for points holds for faces.
//
// Compiled with -ffp-contract=off: the per-pair function is float32 operation by operation, in the header's order.
#include <math.h>

#include "eslam_common.h"

#define TD_THREADS 256
#define TD_PER_THREAD 16
#define TD_CHUNK (TD_THREADS * TD_PER_THREAD)       // scan chunk
#define TD_SCAN_THREADS 1024
#define TD_MAX_BLOCKS (1 << 20)                     // grid-stride loops beyond this many workgroups

static int td_blocks(int64_t n) {
    const int64_t b = (n + TD_THREADS - 1) / TD_THREADS;
    return (int)(b < 1 ? 1 : b > TD_MAX_BLOCKS ? TD_MAX_BLOCKS : b);
}

// ---------------------------------------------------------------------------------------------------------
// in-place exclusive scan of int32 a[0..n), total to a[n] (the scheme of rc_scan, eslam_recon.hip)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void td_scan_chunks_kernel(int32_t* __restrict__ a, int64_t n,
                                                                    int32_t* __restrict__ partial) {
    __shared__ int32_t lds[TD_THREADS / 64];
    const int64_t c0 = (int64_t)blockIdx.x * TD_CHUNK;
    int32_t next = 0;
    for (int k = 0; k < TD_PER_THREAD; ++k) {
        if (c0 + k * TD_THREADS >= n) break;                   // (uniform over the workgroup)
        const int64_t i = c0 + k * TD_THREADS + threadIdx.x;
        const int32_t v = i < n ? a[i] : 0;
        int32_t tot;
        const int32_t off = block_excl_scan<int32_t, TD_THREADS>(v, lds, tot);
        if (i < n) a[i] = next + off;
        next += tot;
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = next;
}

__global__ __launch_bounds__(TD_SCAN_THREADS) void td_scan_partials_kernel(int32_t* __restrict__ partial, int64_t nchunks,
                                                                           int32_t* __restrict__ total) {
    __shared__ int32_t lds[TD_SCAN_THREADS / 64];
    int32_t carry = 0;
    for (int64_t base = 0; base < nchunks; base += TD_SCAN_THREADS) {
        const int64_t c = base + threadIdx.x;
        const int32_t v = c < nchunks ? partial[c] : 0;
        int32_t tot;
        const int32_t e = block_excl_scan<int32_t, TD_SCAN_THREADS>(v, lds, tot);
        if (c < nchunks) partial[c] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(TD_THREADS) void td_scan_add_kernel(int32_t* __restrict__ a, int64_t n,
                                                                 const int32_t* __restrict__ partial) {
    const int64_t c0 = (int64_t)blockIdx.x * TD_CHUNK;
    const int32_t add = partial[blockIdx.x];
    for (int k = 0; k < TD_PER_THREAD; ++k) {
        const int64_t i = c0 + k * TD_THREADS + threadIdx.x;
        if (i < n) a[i] += add;
    }
}

static int64_t td_chunks(int64_t n) { return (n + TD_CHUNK - 1) / TD_CHUNK; }

static int td_scan(int32_t* a, int64_t n, int32_t* partial, hipStream_t st) {
    const int64_t nch = td_chunks(n);
    hipLaunchKernelGGL(td_scan_chunks_kernel, dim3((unsigned)nch), dim3(TD_THREADS), 0, st, a, n, partial);
    if (eslam_check_launch("td_scan_chunks_kernel")) return 1;
    hipLaunchKernelGGL(td_scan_partials_kernel, dim3(1), dim3(TD_SCAN_THREADS), 0, st, partial, nch, a + n);
    if (eslam_check_launch("td_scan_partials_kernel")) return 1;
    hipLaunchKernelGGL(td_scan_add_kernel, dim3((unsigned)nch), dim3(TD_THREADS), 0, st, a, n, partial);
    return eslam_check_launch("td_scan_add_kernel");
}

// ---------------------------------------------------------------------------------------------------------
// the grid
// ---------------------------------------------------------------------------------------------------------
struct TdDev {
    float lox, loy, loz, cell, inv;
    int nx, ny, nz;
};

// clamped in float first: coordinates far outside the box (or NaN, which fmaxf turns into 0) stay in range.  Monotone in
// p, so the cells of a face's box corners bracket the cell of every point of the face.
__device__ __forceinline__ int td_axis_cell(float p, float lo, float inv, int n) {
    const float f = fminf(fmaxf(floorf((p - lo) * inv), 0.0f), (float)(n - 1));
    return (int)f;
}

struct TdFace {
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    int x0, x1, y0, y1, z0, z1;
};

// false: the face is entered nowhere (an index out of range, a non-finite coordinate)
__device__ __forceinline__ bool td_load_face(const float* __restrict__ verts, int64_t n_verts,
                                             const int32_t* __restrict__ faces, int64_t f, const TdDev& g, TdFace& t) {
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return false;
    t.ax = verts[3 * i0]; t.ay = verts[3 * i0 + 1]; t.az = verts[3 * i0 + 2];
    t.bx = verts[3 * i1]; t.by = verts[3 * i1 + 1]; t.bz = verts[3 * i1 + 2];
    t.cx = verts[3 * i2]; t.cy = verts[3 * i2 + 1]; t.cz = verts[3 * i2 + 2];
    // (x - x is 0 for every finite x and NaN otherwise)
    const float z = (t.ax - t.ax) + (t.ay - t.ay) + (t.az - t.az) + (t.bx - t.bx) + (t.by - t.by) + (t.bz - t.bz) +
                    (t.cx - t.cx) + (t.cy - t.cy) + (t.cz - t.cz);
    if (!(z == 0.0f)) return false;
    t.x0 = td_axis_cell(fminf(fminf(t.ax, t.bx), t.cx), g.lox, g.inv, g.nx);
    t.x1 = td_axis_cell(fmaxf(fmaxf(t.ax, t.bx), t.cx), g.lox, g.inv, g.nx);
    t.y0 = td_axis_cell(fminf(fminf(t.ay, t.by), t.cy), g.loy, g.inv, g.ny);
    t.y1 = td_axis_cell(fmaxf(fmaxf(t.ay, t.by), t.cy), g.loy, g.inv, g.ny);
    t.z0 = td_axis_cell(fminf(fminf(t.az, t.bz), t.cz), g.loz, g.inv, g.nz);
    t.z1 = td_axis_cell(fmaxf(fmaxf(t.az, t.bz), t.cz), g.loz, g.inv, g.nz);
    return true;
}

// total[0] += entries, total[1] += faces entered: one 64-bit atomic pair per wave
__global__ __launch_bounds__(TD_THREADS) void td_total_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                              const int32_t* __restrict__ faces, int64_t n_faces,
                                                              const TdDev g, unsigned long long* __restrict__ total) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    long long entries = 0, entered = 0;
    for (int64_t f = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; f < n_faces; f += stride) {
        TdFace t;
        if (!td_load_face(verts, n_verts, faces, f, g, t)) continue;
        entries += (long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) * (t.z1 - t.z0 + 1);
        entered += 1;
    }
    for (int off = 32; off > 0; off >>= 1) {
        entries += __shfl_down(entries, off, 64);
        entered += __shfl_down(entered, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && entered) {
        atomicAdd(&total[0], (unsigned long long)entries);
        atomicAdd(&total[1], (unsigned long long)entered);
    }
}

__global__ __launch_bounds__(TD_THREADS) void td_count_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                              const int32_t* __restrict__ faces, int64_t n_faces,
                                                              const TdDev g, int32_t* __restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    for (int64_t f = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; f < n_faces; f += stride) {
        TdFace t;
        if (!td_load_face(verts, n_verts, faces, f, g, t)) continue;
        for (int ix = t.x0; ix <= t.x1; ++ix)
            for (int iy = t.y0; iy <= t.y1; ++iy)
                for (int iz = t.z0; iz <= t.z1; ++iz) atomicAdd(&counts[(ix * g.ny + iy) * g.nz + iz], 1);
    }
}

// ends[c] holds cell c's start on entry and its end on exit.  `capacity` = the entries the workspace was sized for: a
// position beyond it (a grid->entries that is not this mesh's count) is dropped, never written.
__global__ __launch_bounds__(TD_THREADS) void td_fill_kernel(const float* __restrict__ verts, int64_t n_verts,
                                                             const int32_t* __restrict__ faces, int64_t n_faces,
                                                             const TdDev g, int32_t* __restrict__ ends, int64_t capacity,
                                                             float4* __restrict__ rec) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    for (int64_t f = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; f < n_faces; f += stride) {
        TdFace t;
        if (!td_load_face(verts, n_verts, faces, f, g, t)) continue;
        const float4 r0 = make_float4(t.ax, t.ay, t.az, __int_as_float((int)f));
        const float4 r1 = make_float4(t.bx, t.by, t.bz, 0.0f);
        const float4 r2 = make_float4(t.cx, t.cy, t.cz, 0.0f);
        for (int ix = t.x0; ix <= t.x1; ++ix)
            for (int iy = t.y0; iy <= t.y1; ++iy)
                for (int iz = t.z0; iz <= t.z1; ++iz) {
                    const int64_t pos = atomicAdd(&ends[(ix * g.ny + iy) * g.nz + iz], 1);
                    if (pos < 0 || pos >= capacity) continue;
                    rec[3 * pos] = r0;
                    rec[3 * pos + 1] = r1;
                    rec[3 * pos + 2] = r2;
                }
    }
}

// ---------------------------------------------------------------------------------------------------------
// counting sort of the queries into cell order
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TD_THREADS) void td_query_count_kernel(const float* __restrict__ pts, int64_t n, const TdDev g,
                                                                    int32_t* __restrict__ counts, int32_t* __restrict__ cell,
                                                                    int32_t* __restrict__ slot) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; i < n; i += stride) {
        const int ix = td_axis_cell(pts[3 * i], g.lox, g.inv, g.nx), iy = td_axis_cell(pts[3 * i + 1], g.loy, g.inv, g.ny);
        const int iz = td_axis_cell(pts[3 * i + 2], g.loz, g.inv, g.nz);
        const int c = (ix * g.ny + iy) * g.nz + iz;
        cell[i] = c;
        slot[i] = atomicAdd(&counts[c], 1);
    }
}

__global__ __launch_bounds__(TD_THREADS) void td_query_order_kernel(int64_t n, const int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ cell,
                                                                    const int32_t* __restrict__ slot,
                                                                    int32_t* __restrict__ order) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; i < n; i += stride)
        order[(int64_t)start[cell[i]] + slot[i]] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------------------
// the per-pair function (include/eslam_hip.h states the order; tests/meshdist_ref.py mirrors it)
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float td_dot(float ux, float uy, float uz, float vx, float vy, float vz) {
    return ux * vx + uy * vy + uz * vz;
}

__device__ __forceinline__ float td_norm1(float x, float y, float z) { return fabsf(x) + fabsf(y) + fabsf(z); }

__device__ __forceinline__ bool td_divisor_ok(float s) { return s > 0.0f && s < INFINITY; }

// the nearest point of segment o + t e, t in [0, 1], kept when strictly nearer than (bd2, bx, by, bz)
__device__ __forceinline__ void td_segment(float ox, float oy, float oz, float ex, float ey, float ez, float qx, float qy,
                                           float qz, float& bd2, float& bx, float& by, float& bz) {
    const float ee = td_dot(ex, ey, ez, ex, ey, ez);
    float t = 0.0f;
    if (td_divisor_ok(ee)) t = fminf(fmaxf(td_dot(qx - ox, qy - oy, qz - oz, ex, ey, ez) / ee, 0.0f), 1.0f);
    const float px = ox + ex * t, py = oy + ey * t, pz = oz + ez * t;
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float d2 = td_dot(dx, dy, dz, dx, dy, dz);
    if (d2 < bd2) {
        bd2 = d2;
        bx = px; by = py; bz = pz;
    }
}

__device__ __forceinline__ void td_closest(const float4 A, const float4 B, const float4 C, float qx, float qy, float qz,
                                           float& px, float& py, float& pz) {
    const float ax = A.x, ay = A.y, az = A.z;
    const float abx = B.x - ax, aby = B.y - ay, abz = B.z - az, acx = C.x - ax, acy = C.y - ay, acz = C.z - az;
    const float apx = qx - ax, apy = qy - ay, apz = qz - az;
    const float d1 = td_dot(abx, aby, abz, apx, apy, apz), d2 = td_dot(acx, acy, acz, apx, apy, apz);
    px = ax; py = ay; pz = az;
    if (d1 <= 0.0f && d2 <= 0.0f) return;                                           // vertex A
    const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const float d3 = td_dot(abx, aby, abz, bpx, bpy, bpz), d4 = td_dot(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) {                                                   // vertex B
        px = B.x; py = B.y; pz = B.z;
        return;
    }
    float s;
    bool decided = false;
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {                                   // edge AB
        s = d1 - d3;
        if (td_divisor_ok(s)) {
            const float v = d1 / s;
            px = ax + abx * v; py = ay + aby * v; pz = az + abz * v;
            return;
        }
        decided = true;
    }
    float d5 = 0.0f, d6 = 0.0f, vb = 0.0f;
    if (!decided) {
        const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
        d5 = td_dot(abx, aby, abz, cpx, cpy, cpz);
        d6 = td_dot(acx, acy, acz, cpx, cpy, cpz);
        if (d6 >= 0.0f && d5 <= d6) {                                               // vertex C
            px = C.x; py = C.y; pz = C.z;
            return;
        }
        vb = d5 * d2 - d1 * d6;
        if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {                               // edge AC
            s = d2 - d6;
            if (td_divisor_ok(s)) {
                const float w = d2 / s;
                px = ax + acx * w; py = ay + acy * w; pz = az + acz * w;
                return;
            }
            decided = true;
        }
    }
    if (!decided) {
        const float va = d3 * d6 - d5 * d4;
        const float e43 = d4 - d3, e56 = d5 - d6;
        if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {                             // edge BC
            s = e43 + e56;
            if (td_divisor_ok(s)) {
                const float w = e43 / s;
                px = B.x + (C.x - B.x) * w; py = B.y + (C.y - B.y) * w; pz = B.z + (C.z - B.z) * w;
                return;
            }
        } else {                                                                    // interior
            // va, vb, vc are differences of products: below their rounding noise (thin faces) the weights would be
            // arbitrary, so the interior is taken only where all three stand clear of it
            const float nab = td_norm1(abx, aby, abz), nac = td_norm1(acx, acy, acz);
            const float m = (td_norm1(apx, apy, apz) + nab) + nac;
            const float tol = (1e-6f * (nab * nac)) * (m * m);
            s = (va + vb) + vc;
            if (va > tol && vb > tol && vc > tol && td_divisor_ok(s)) {
                const float r = 1.0f / s;
                const float v = vb * r, w = vc * r;
                px = (ax + abx * v) + acx * w; py = (ay + aby * v) + acy * w; pz = (az + abz * v) + acz * w;
                return;
            }
        }
    }
    // a divisor that is not positive and finite, or an interior within the noise: the nearest of the three segments (A
    // when none compares)
    float bd2 = INFINITY;
    td_segment(ax, ay, az, abx, aby, abz, qx, qy, qz, bd2, px, py, pz);
    td_segment(ax, ay, az, acx, acy, acz, qx, qy, qz, bd2, px, py, pz);
    td_segment(B.x, B.y, B.z, C.x - B.x, C.y - B.y, C.z - B.z, qx, qy, qz, bd2, px, py, pz);
}

// distance from q to the slab [lo, lo + cell] along one axis, less the slack (never negative)
__device__ __forceinline__ float td_gap(float q, float lo, float cell, float slack) {
    return fmaxf(fmaxf(lo - q, q - (lo + cell)) - slack, 0.0f);
}

// One query per lane, in cell order when `order` is given; the ring search and its stopping bound are nn_query_kernel's.
// The slack also covers the rounding of the per-pair function: its point is, to a few ulps of the coordinates, a point
// of the face, so its distance is not below the face's true distance by more than that.
// best: (d2, face) minimised lexicographically; a face met again in another cell compares equal and changes nothing.
__global__ __launch_bounds__(TD_THREADS) void td_query_kernel(const float* __restrict__ qs, int64_t nq,
                                                              const int32_t* __restrict__ order, const TdDev g,
                                                              const int32_t* __restrict__ ends,
                                                              const float4* __restrict__ rec, int capacity, float limit2,
                                                              float max_dist, float* __restrict__ dist,
                                                              int32_t* __restrict__ face,
                                                              float* __restrict__ closest) {
    const int64_t stride = (int64_t)gridDim.x * TD_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x; t < nq; t += stride) {
        const int64_t qi = order ? (int64_t)order[t] : t;
        const float qx = qs[3 * qi], qy = qs[3 * qi + 1], qz = qs[3 * qi + 2];
        float best = limit2, bpx = NAN, bpy = NAN, bpz = NAN;
        int bi = -1;
        const bool finite = ((qx - qx) + (qy - qy) + (qz - qz)) == 0.0f;
        const int cx = td_axis_cell(qx, g.lox, g.inv, g.nx), cy = td_axis_cell(qy, g.loy, g.inv, g.ny);
        const int cz = td_axis_cell(qz, g.loz, g.inv, g.nz);
        const float hix = g.lox + g.nx * g.cell, hiy = g.loy + g.ny * g.cell, hiz = g.loz + g.nz * g.cell;
        const float mag = fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)) +
                          fmaxf(fmaxf(fmaxf(fabsf(g.lox), fabsf(hix)), fmaxf(fabsf(g.loy), fabsf(hiy))),
                                fmaxf(fabsf(g.loz), fabsf(hiz)));
        const float slack = 4e-6f * mag;
        for (int r = 0; finite; ++r) {
            const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r, z0 = cz - r, z1 = cz + r;
            const int zlo = max(z0, 0), zhi = min(z1, g.nz - 1);
            for (int ix = max(x0, 0); ix <= min(x1, g.nx - 1); ++ix) {
                const bool xe = ix == x0 || ix == x1;
                const float gx = td_gap(qx, g.lox + ix * g.cell, g.cell, slack);
                for (int iy = max(y0, 0); iy <= min(y1, g.ny - 1); ++iy) {
                    const bool ye = iy == y0 || iy == y1;
                    const float gy = td_gap(qy, g.loy + iy * g.cell, g.cell, slack);
                    const float gxy = gx * gx + gy * gy;
                    if (gxy >= best) continue;
                    const int step = (xe || ye) ? 1 : max(z1 - z0, 1);   // inner cells: only the two z faces
                    for (int iz = (xe || ye) ? zlo : z0; iz <= zhi; iz += step) {
                        if (iz < 0) continue;
                        const float gz = td_gap(qz, g.loz + iz * g.cell, g.cell, slack);
                        if (gxy + gz * gz >= best) continue;
                        const int c = (ix * g.ny + iy) * g.nz + iz;
                        const int j1 = min(ends[c], capacity);             // (never past the records the build wrote)
                        for (int j = c > 0 ? max(ends[c - 1], 0) : 0; j < j1; ++j) {
                            const float4 A = rec[3 * (int64_t)j], B = rec[3 * (int64_t)j + 1], C = rec[3 * (int64_t)j + 2];
                            float px, py, pz;
                            td_closest(A, B, C, qx, qy, qz, px, py, pz);
                            const float dx = qx - px, dy = qy - py, dz = qz - pz;
                            const float d2 = td_dot(dx, dy, dz, dx, dy, dz);
                            const int fi = __float_as_int(A.w);
                            if (d2 < best || (d2 == best && fi < bi)) {
                                best = d2;
                                bi = fi;
                                bpx = px; bpy = py; bpz = pz;
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
        if (bi < 0) bpx = bpy = bpz = NAN;
        dist[qi] = d;
        face[qi] = bi;
        if (closest) {
            closest[3 * qi] = bpx;
            closest[3 * qi + 1] = bpy;
            closest[3 * qi + 2] = bpz;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static int64_t td_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

static bool td_grid_ok(const char* who, const eslam_tri_grid_t* g) {
    if (!g) {
        eslam_set_error("%s: null grid", who);
        return false;
    }
    const double cells = (double)g->dims[0] * g->dims[1] * g->dims[2];
    if (g->dims[0] < 1 || g->dims[1] < 1 || g->dims[2] < 1 || cells > ESLAM_TRI_MAX_CELLS || !(g->cell > 0.0f) ||
        !isfinite(g->cell) || !isfinite(g->lo[0]) || !isfinite(g->lo[1]) || !isfinite(g->lo[2])) {
        eslam_set_error("%s: invalid grid (%d x %d x %d cells of %g)", who, g->dims[0], g->dims[1], g->dims[2],
                        (double)g->cell);
        return false;
    }
    return true;
}

static bool td_entries_ok(const char* who, const eslam_tri_grid_t* g) {
    if (g->entries < 0 || g->entries > ESLAM_TRI_MAX_ENTRIES) {
        eslam_set_error("%s: %lld (face, cell) entries, at most 2^31 - 1: a few faces far larger than the others span "
                        "most of the %d x %d x %d cells", who, (long long)g->entries, g->dims[0], g->dims[1], g->dims[2]);
        return false;
    }
    return true;
}

static bool td_mesh_ok(const char* who, const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces) {
    if (n_verts < 0 || n_verts > INT32_MAX || n_faces < 0 || n_faces > INT32_MAX) {
        eslam_set_error("%s: %lld vertices, %lld faces (0 .. 2^31 - 1)", who, (long long)n_verts, (long long)n_faces);
        return false;
    }
    if (n_faces > 0 && (!verts || !faces || n_verts < 1)) {
        eslam_set_error("%s: %lld faces over %lld vertices, or a null argument", who, (long long)n_faces, (long long)n_verts);
        return false;
    }
    return true;
}

static int64_t td_cells(const eslam_tri_grid_t* g) { return (int64_t)g->dims[0] * g->dims[1] * g->dims[2]; }

static TdDev td_dev(const eslam_tri_grid_t* g) {
    TdDev d;
    d.lox = g->lo[0]; d.loy = g->lo[1]; d.loz = g->lo[2];
    d.cell = g->cell; d.inv = 1.0f / g->cell;
    d.nx = g->dims[0]; d.ny = g->dims[1]; d.nz = g->dims[2];
    return d;
}

extern "C" int eslam_tri_grid_plan(int64_t n_faces, const float* bbox6_host, float face_extent, eslam_tri_grid_t* grid) {
    if (n_faces < 0 || n_faces > INT32_MAX || !grid || (n_faces > 0 && !bbox6_host)) {
        eslam_set_error("eslam_tri_grid_plan: %lld faces (0 .. 2^31 - 1) or a null argument", (long long)n_faces);
        return 1;
    }
    grid->reserved = 0;
    grid->entries = 0;
    grid->cell = 1.0f;
    grid->dims[0] = grid->dims[1] = grid->dims[2] = 1;
    grid->lo[0] = grid->lo[1] = grid->lo[2] = 0.0f;
    if (n_faces == 0) return 0;
    double ext[3], E = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double lo = bbox6_host[2 * d], hi = bbox6_host[2 * d + 1];
        if (!isfinite(lo) || !isfinite(hi) || hi < lo) {
            eslam_set_error("eslam_tri_grid_plan: bad bounding box on axis %d: [%g, %g]", d, lo, hi);
            return 1;
        }
        ext[d] = hi - lo;
        E = fmax(E, ext[d]);
        grid->lo[d] = bbox6_host[2 * d];
    }
    if (!(E > 0.0)) return 0;                           // all vertices equal: one cell
    int m = 0;
    double vol = 1.0;
    for (int d = 0; d < 3; ++d)
        if (ext[d] > 1e-6 * E) {                        // flat axes (extent <= 1e-6 of the largest) get one cell
            ++m;
            vol *= ext[d];
        }
    double cell = face_extent > 0.0f && isfinite(face_extent) ? ESLAM_TRI_CELL_PER_EXTENT * (double)face_extent
                                                              : pow(vol / (double)n_faces, 1.0 / m);
    cell = fmax(cell, pow(vol / (double)ESLAM_TRI_MAX_CELLS, 1.0 / m));
    for (;;) {
        const float cf = nextafterf((float)cell, INFINITY);     // dims * cf covers the extent
        double prod = 1.0;
        int dims[3];
        for (int d = 0; d < 3; ++d) {
            const double n = fmax(1.0, ceil(ext[d] / (double)cf));
            prod *= n;
            dims[d] = n > ESLAM_TRI_MAX_CELLS ? ESLAM_TRI_MAX_CELLS + 1 : (int)n;
        }
        if (prod <= ESLAM_TRI_MAX_CELLS) {
            grid->cell = cf;
            for (int d = 0; d < 3; ++d) grid->dims[d] = dims[d];
            return 0;
        }
        cell *= 1.1;
    }
}

extern "C" int eslam_tri_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                               const eslam_tri_grid_t* grid, int64_t* total, eslam_stream_t stream) {
    if (!td_grid_ok("eslam_tri_count", grid) || !td_mesh_ok("eslam_tri_count", verts, n_verts, faces, n_faces)) return 1;
    if (!total) {
        eslam_set_error("eslam_tri_count: null total");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(total, 0, 16, st) != hipSuccess) {
        eslam_set_error("eslam_tri_count: memset failed");
        return 2;
    }
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(td_total_kernel, dim3(td_blocks(n_faces)), dim3(TD_THREADS), 0, st, verts, n_verts, faces, n_faces,
                       td_dev(grid), (unsigned long long*)total);
    return eslam_check_launch("td_total_kernel");
}

struct TdWork {
    int32_t* ends;       // [cells + 1]
    int32_t* partial;    // [chunks(cells + 1)]
    float4* rec;         // [3 entries]
};

static int64_t td_work_layout(int64_t cells, int64_t entries, void* base, TdWork* w) {
    char* p = (char*)base;
    int64_t off = 0;
    if (w) w->ends = (int32_t*)(p + off);
    off += td_align(4 * (cells + 1));
    if (w) w->partial = (int32_t*)(p + off);
    off += td_align(4 * td_chunks(cells + 1));
    if (w) w->rec = (float4*)(p + off);
    off += td_align(48 * entries);
    return off;
}

struct TdQueryWork {
    int32_t* start;      // [cells + 1]
    int32_t* partial;    // [chunks(cells + 1)]
    int32_t* cell;       // [n]
    int32_t* slot;       // [n]
    int32_t* order;      // [n]
};

static int64_t td_query_layout(int64_t cells, int64_t n, void* base, TdQueryWork* w) {
    char* p = (char*)base;
    int64_t off = 0;
    if (w) w->start = (int32_t*)(p + off);
    off += td_align(4 * (cells + 1));
    if (w) w->partial = (int32_t*)(p + off);
    off += td_align(4 * td_chunks(cells + 1));
    if (w) w->cell = (int32_t*)(p + off);
    off += td_align(4 * n);
    if (w) w->slot = (int32_t*)(p + off);
    off += td_align(4 * n);
    if (w) w->order = (int32_t*)(p + off);
    off += td_align(4 * n);
    return off;
}

extern "C" int64_t eslam_tri_workspace_bytes(const eslam_tri_grid_t* grid) {
    if (!td_grid_ok("eslam_tri_workspace_bytes", grid) || !td_entries_ok("eslam_tri_workspace_bytes", grid)) return -1;
    return td_work_layout(td_cells(grid), grid->entries, nullptr, nullptr);
}

extern "C" int64_t eslam_tri_query_workspace_bytes(const eslam_tri_grid_t* grid, int64_t n_query) {
    if (!td_grid_ok("eslam_tri_query_workspace_bytes", grid)) return -1;
    if (n_query < 0 || n_query > INT32_MAX) {
        eslam_set_error("eslam_tri_query_workspace_bytes: %lld queries (0 .. 2^31 - 1)", (long long)n_query);
        return -1;
    }
    return td_query_layout(td_cells(grid), n_query, nullptr, nullptr);
}

extern "C" int eslam_tri_build(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                               const eslam_tri_grid_t* grid, void* workspace, eslam_stream_t stream) {
    if (!td_grid_ok("eslam_tri_build", grid) || !td_entries_ok("eslam_tri_build", grid) ||
        !td_mesh_ok("eslam_tri_build", verts, n_verts, faces, n_faces))
        return 1;
    if (n_faces == 0 || grid->entries == 0) return 0;              // nothing is entered: queries launch nothing either
    if (!workspace) {
        eslam_set_error("eslam_tri_build: null workspace");
        return 1;
    }
    const TdDev g = td_dev(grid);
    const int64_t cells = td_cells(grid);
    TdWork w;
    td_work_layout(cells, grid->entries, workspace, &w);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(w.ends, 0, (size_t)(cells + 1) * 4, st) != hipSuccess) {
        eslam_set_error("eslam_tri_build: memset failed");
        return 2;
    }
    hipLaunchKernelGGL(td_count_kernel, dim3(td_blocks(n_faces)), dim3(TD_THREADS), 0, st, verts, n_verts, faces, n_faces, g,
                       w.ends);
    if (eslam_check_launch("td_count_kernel")) return 1;
    if (int rc = td_scan(w.ends, cells, w.partial, st)) return rc;
    hipLaunchKernelGGL(td_fill_kernel, dim3(td_blocks(n_faces)), dim3(TD_THREADS), 0, st, verts, n_verts, faces, n_faces, g,
                       w.ends, grid->entries, w.rec);
    return eslam_check_launch("td_fill_kernel");
}

extern "C" int eslam_tri_query(const eslam_tri_grid_t* grid, const void* workspace, const float* queries, int64_t n_query,
                               float max_dist, int flags, void* query_workspace, float* dist, int32_t* face, float* closest,
                               eslam_stream_t stream) {
    if (!td_grid_ok("eslam_tri_query", grid) || !td_entries_ok("eslam_tri_query", grid)) return 1;
    if (n_query < 0 || n_query > INT32_MAX) {
        eslam_set_error("eslam_tri_query: %lld queries (0 .. 2^31 - 1)", (long long)n_query);
        return 1;
    }
    if (flags & ~ESLAM_TRI_INPUT_ORDER) {
        eslam_set_error("eslam_tri_query: unknown flags 0x%x", flags);
        return 1;
    }
    if (isnan(max_dist)) {
        eslam_set_error("eslam_tri_query: NaN max_dist");
        return 1;
    }
    if (n_query == 0 || grid->entries == 0) return 0;
    const bool input_order = flags & ESLAM_TRI_INPUT_ORDER;
    if (!workspace || !queries || !dist || !face || (!input_order && !query_workspace)) {
        eslam_set_error("eslam_tri_query: null argument");
        return 1;
    }
    const TdDev g = td_dev(grid);
    const int64_t cells = td_cells(grid);
    TdWork w;
    td_work_layout(cells, grid->entries, const_cast<void*>(workspace), &w);
    hipStream_t st = (hipStream_t)stream;
    const int32_t* order = nullptr;
    if (!input_order) {
        TdQueryWork q;
        td_query_layout(cells, n_query, query_workspace, &q);
        if (hipMemsetAsync(q.start, 0, (size_t)(cells + 1) * 4, st) != hipSuccess) {
            eslam_set_error("eslam_tri_query: memset failed");
            return 2;
        }
        hipLaunchKernelGGL(td_query_count_kernel, dim3(td_blocks(n_query)), dim3(TD_THREADS), 0, st, queries, n_query, g,
                           q.start, q.cell, q.slot);
        if (eslam_check_launch("td_query_count_kernel")) return 1;
        if (int rc = td_scan(q.start, cells, q.partial, st)) return rc;
        hipLaunchKernelGGL(td_query_order_kernel, dim3(td_blocks(n_query)), dim3(TD_THREADS), 0, st, n_query, q.start, q.cell,
                           q.slot, q.order);
        if (eslam_check_launch("td_query_order_kernel")) return 1;
        order = q.order;
    }
    // candidates must have d2 < limit2; a little above max_dist^2 so that the exact test sqrt(d2) < max_dist decides
    const float limit2 = isinf(max_dist) ? INFINITY : max_dist * max_dist * (1.0f + 1e-6f);
    hipLaunchKernelGGL(td_query_kernel, dim3(td_blocks(n_query)), dim3(TD_THREADS), 0, st, queries, n_query, order, g, w.ends,
                       w.rec, (int)grid->entries, limit2, max_dist, dist, face, closest);
    return eslam_check_launch("td_query_kernel");
}
