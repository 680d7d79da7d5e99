// TSDF fusion of RGB-D frames into a dense volume [nx][ny][nz] (z fastest, the layout eslam_mc_* takes): replaces the
// integrate step of open3d's ScalableTSDFVolume in reference src/utils/Mesher.py:63-128.  The per-voxel rule is in
// include/eslam_hip.h (eslam_tsdf_integrate) and DESIGN.md section 17; every operation of it is float32, in the order
// written there, and this file is built with -ffp-contract=off so that tests/tsdf_ref.py can mirror it bit for bit.
//
// Shape: a wave owns a run of 64 z-consecutive voxels (one coalesced 256 B access per array) and walks the frames of the
// call in index order with tsdf, weight and colour in registers, so the volume is read and written once per call and not
// once per frame.  Two tests keep a run away from frames, and from memory, it has nothing to do with:
//   run test    lane f takes frame f (64 frames at a time): both ends of the run in the camera frame against the near
//               plane, depth_max[f] + trunc and the four sides of the image, each widened by a margin that covers the
//               float32 rounding of the per-voxel arithmetic (and one pixel on the sides).  A frame is dropped only when
//               both ends are outside the same plane (the run is a segment, so then all of it is).  The ballot of the
//               survivors is the run's frame mask;
//   voxel rule  for the frames of the mask, poses read wave-uniformly (scalar loads), each lane applies the rule itself.
// The run test only ever drops frames the rule would skip for all 64 voxels (it is conservative); the rule is what
// decides, so the result does not depend on the test.  A run is loaded at the first frame that updates one of its voxels
// and stored at the end when it was loaded: a run that no frame of the call updates is neither read nor written.
// No atomics: a voxel belongs to one lane.
#include "eslam_common.h"

#define TSDF_THREADS 256
#define TSDF_WAVES (TSDF_THREADS / WAVE)

struct TsdfGrid {
    int64_t nx, ny, nz, nzr, runs;     // nzr = runs of 64 along z per (x, y) column; runs = nx * ny * nzr
    float origin[3], voxel, trunc;
};

struct TsdfCam {
    float fx, fy, cx, cy;
    int H, W, n_frames;
};

// both ends (a, b) of a run outside the half-space l >= 0, with margin m
__device__ __forceinline__ bool tsdf_both_below(float la, float lb, float m) { return la < -m && lb < -m; }

template <bool COLOR>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                      float* __restrict__ color, const TsdfGrid g,
                                                                      const TsdfCam cam, const float* __restrict__ depths,
                                                                      const float* __restrict__ colors,
                                                                      const float* __restrict__ w2c,
                                                                      const float* __restrict__ depth_max) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t run = (int64_t)blockIdx.x * TSDF_WAVES + (threadIdx.x >> 6);
    if (run >= g.runs) return;                                   // (uniform over the wave)
    const int64_t col = run / g.nzr, zr = run - col * g.nzr;
    const int64_t ix = col / g.ny, iy = col - ix * g.ny;
    const int64_t iz0 = zr * WAVE, iz = iz0 + lane;
    const int64_t iz1 = iz0 + WAVE - 1 < g.nz ? iz0 + WAVE - 1 : g.nz - 1;
    const bool active = iz < g.nz;
    const int64_t vi = col * g.nz + iz;
    const float px = g.origin[0] + ((float)ix + 0.5f) * g.voxel;
    const float py = g.origin[1] + ((float)iy + 0.5f) * g.voxel;
    const float pz = g.origin[2] + ((float)iz + 0.5f) * g.voxel;
    const float pza = g.origin[2] + ((float)iz0 + 0.5f) * g.voxel;
    const float pzb = g.origin[2] + ((float)iz1 + 0.5f) * g.voxel;
    const float fW = (float)cam.W, fH = (float)cam.H;
    const int64_t npix = (int64_t)cam.H * cam.W;

    bool loaded = false;
    float tv = 0.0f, wv = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;

    for (int f0 = 0; f0 < cam.n_frames; f0 += WAVE) {
        // ---- run test: lane f takes frame f0 + f ----
        bool may = false;
        const int f = f0 + lane;
        if (f < cam.n_frames) {
            const float* m = w2c + (int64_t)f * 12;
            float ca[3], cb[3], s[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float xy = m[4 * r] * px + m[4 * r + 1] * py;
                ca[r] = (xy + m[4 * r + 2] * pza) + m[4 * r + 3];
                cb[r] = (xy + m[4 * r + 2] * pzb) + m[4 * r + 3];
                s[r] = (fabsf(m[4 * r] * px) + fabsf(m[4 * r + 1] * py)) +
                       (fmaxf(fabsf(m[4 * r + 2] * pza), fabsf(m[4 * r + 2] * pzb)) + fabsf(m[4 * r + 3]));
            }
            // a camera coordinate of any voxel of the run is within 2^-19 s[r] of the segment ca[r]..cb[r] (six roundings of
            // 2^-24 each on terms that sum to s[r], for the voxel and for the ends, and the voxel's own rounded z); the
            // margins are 2^-18 s[r] and up
            const float ez = s[2] * 3.8146973e-6f;
            const float ex = cam.fx * (s[0] * 3.8146973e-6f) + (fabsf(cam.cx) + fW + 2.0f) * ez;
            const float ey = cam.fy * (s[1] * 3.8146973e-6f) + (fabsf(cam.cy) + fH + 2.0f) * ez;
            const float dm = depth_max[f];
            bool out = tsdf_both_below(ca[2], cb[2], ez);                                          // behind the camera
            out |= tsdf_both_below((dm + g.trunc) - ca[2], (dm + g.trunc) - cb[2], ez);         // beyond depth_max + trunc
            // sides, one pixel wider than floor(u + 0.5) in [0, W): u + 1.5 >= 0 and u - 0.5 <= W, times c.z > 0
            out |= tsdf_both_below(cam.fx * ca[0] + (cam.cx + 1.5f) * ca[2], cam.fx * cb[0] + (cam.cx + 1.5f) * cb[2], ex);
            out |= tsdf_both_below((fW + 0.5f - cam.cx) * ca[2] - cam.fx * ca[0], (fW + 0.5f - cam.cx) * cb[2] - cam.fx * cb[0], ex);
            out |= tsdf_both_below(cam.fy * ca[1] + (cam.cy + 1.5f) * ca[2], cam.fy * cb[1] + (cam.cy + 1.5f) * cb[2], ey);
            out |= tsdf_both_below((fH + 0.5f - cam.cy) * ca[2] - cam.fy * ca[1], (fH + 0.5f - cam.cy) * cb[2] - cam.fy * cb[1], ey);
            may = !out;                       // (a NaN anywhere compares false: the frame stays)
        }
        unsigned long long mask = __ballot(may);

        // ---- voxel rule, frames of the mask in index order ----
        while (mask) {
            const int k = f0 + __builtin_ctzll(mask);               // wave-uniform
            mask &= mask - 1;
            const float* m = w2c + (int64_t)k * 12;
            const float cx_ = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
            const float cy_ = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
            const float cz_ = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
            bool upd = active && cz_ > 0.0f;
            const float u = (cam.fx * cx_) / cz_ + cam.cx;
            const float v = (cam.fy * cy_) / cz_ + cam.cy;
            const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
            upd = upd && fu >= 0.0f && fu < fW && fv >= 0.0f && fv < fH;
            float tt = 0.0f;
            int64_t pix = 0;
            if (upd) {
                pix = (int64_t)k * npix + (int64_t)fv * cam.W + (int64_t)fu;
                const float d = depths[pix];
                const float xn = (fu - cam.cx) / cam.fx, yn = (fv - cam.cy) / cam.fy;
                const float len = sqrtf((1.0f + xn * xn) + yn * yn);
                const float sdf = (d - cz_) * len;
                upd = d > 0.0f && sdf > -g.trunc;
                tt = fminf(1.0f, sdf / g.trunc);
            }
            if (__ballot(upd) == 0ull) continue;                    // (uniform)
            if (!loaded) {
                loaded = true;
                if (active) {
                    tv = tsdf[vi];
                    wv = weight[vi];
                    if (COLOR) {
                        c0 = color[vi * 3];
                        c1 = color[vi * 3 + 1];
                        c2 = color[vi * 3 + 2];
                    }
                }
            }
            if (upd) {
                const float w1 = wv + 1.0f;
                tv = (tv * wv + tt) / w1;
                if (COLOR) {
                    const float* cp = colors + pix * 3;
                    c0 = (c0 * wv + cp[0]) / w1;
                    c1 = (c1 * wv + cp[1]) / w1;
                    c2 = (c2 * wv + cp[2]) / w1;
                }
                wv = w1;
            }
        }
    }
    if (loaded && active) {
        tsdf[vi] = tv;
        weight[vi] = wv;
        if (COLOR) {
            color[vi * 3] = c0;
            color[vi * 3 + 1] = c1;
            color[vi * 3 + 2] = c2;
        }
    }
}

// out [n,3] = the colour volume sampled trilinearly at pts [n,3] (world): g = (p - origin) / voxel - 0.5 per axis is the
// position in voxel-centre coordinates, i0 = floor(g), t = g - i0, both indices clamped to the volume
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_sample_color_kernel(const float* __restrict__ color, const TsdfGrid g,
                                                                         const float* __restrict__ pts, int64_t n,
                                                                         float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t dims[3] = {g.nx, g.ny, g.nz};
    int64_t lo[3], hi[3];
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = (pts[i * 3 + a] - g.origin[a]) / g.voxel - 0.5f;
        const float fl = floorf(x);
        t[a] = x - fl;
        // (a NaN or a far-away coordinate: the clamp keeps the indices inside, the value is then meaningless but safe)
        const float top = (float)(dims[a] - 1);
        const float l = fminf(fmaxf(fl, 0.0f), top), h = fminf(fmaxf(fl + 1.0f, 0.0f), top);
        lo[a] = (l == l) ? (int64_t)l : 0;
        hi[a] = (h == h) ? (int64_t)h : 0;
    }
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
        const float w = ((c & 1) ? t[0] : 1.0f - t[0]) * ((c & 2) ? t[1] : 1.0f - t[1]) * ((c & 4) ? t[2] : 1.0f - t[2]);
        const float* p = color + ((x * g.ny + y) * g.nz + z) * 3;
        acc[0] += w * p[0];
        acc[1] += w * p[1];
        acc[2] += w * p[2];
    }
    out[i * 3] = acc[0];
    out[i * 3 + 1] = acc[1];
    out[i * 3 + 2] = acc[2];
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool tsdf_grid(const char* who, int64_t nx, int64_t ny, int64_t nz, const float* origin3_host, float voxel, TsdfGrid& g) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > ((int64_t)1 << 40) / ny / nz) {
        eslam_set_error("%s: volume %lld x %lld x %lld is empty or too large", who, (long long)nx, (long long)ny, (long long)nz);
        return false;
    }
    if (!origin3_host || !(voxel > 0.0f)) {
        eslam_set_error("%s: null origin or voxel size %g not positive", who, (double)voxel);
        return false;
    }
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.nzr = (nz + WAVE - 1) / WAVE;
    g.runs = nx * ny * g.nzr;
    for (int d = 0; d < 3; ++d) g.origin[d] = origin3_host[d];
    g.voxel = voxel;
    g.trunc = 0.0f;
    return true;
}

extern "C" int eslam_tsdf_integrate(float* tsdf, float* weight, float* color, int64_t nx, int64_t ny, int64_t nz,
                                    const float* origin3_host, float voxel, float trunc, const float* depths,
                                    const float* colors, const float* w2c, const float* depth_max, int n_frames, int H, int W,
                                    float fx, float fy, float cx, float cy, eslam_stream_t stream) {
    TsdfGrid g;
    if (!tsdf_grid("eslam_tsdf_integrate", nx, ny, nz, origin3_host, voxel, g)) return 1;
    if (!(trunc > 0.0f) || n_frames < 0 || H < 1 || W < 1 || H > 16384 || W > 16384) {
        eslam_set_error("eslam_tsdf_integrate: trunc %g, %d frames or image %d x %d out of range", (double)trunc, n_frames, W, H);
        return 1;
    }
    if ((color == nullptr) != (colors == nullptr)) {
        eslam_set_error("eslam_tsdf_integrate: the colour volume and the colour images come together or not at all");
        return 1;
    }
    if (n_frames == 0) return 0;
    if (!tsdf || !weight || !depths || !w2c || !depth_max) {
        eslam_set_error("eslam_tsdf_integrate: null argument");
        return 1;
    }
    const int64_t blocks = (g.runs + TSDF_WAVES - 1) / TSDF_WAVES;
    if (blocks > 0x7fffffff) {
        eslam_set_error("eslam_tsdf_integrate: %lld runs of 64 voxels exceed the grid limit", (long long)g.runs);
        return 1;
    }
    g.trunc = trunc;
    TsdfCam cam;
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    cam.H = H; cam.W = W; cam.n_frames = n_frames;
    hipStream_t st = (hipStream_t)stream;
    if (color)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3((unsigned)blocks), dim3(TSDF_THREADS), 0, st, tsdf, weight, color, g,
                           cam, depths, colors, w2c, depth_max);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3((unsigned)blocks), dim3(TSDF_THREADS), 0, st, tsdf, weight, color, g,
                           cam, depths, colors, w2c, depth_max);
    return eslam_check_launch("tsdf_integrate_kernel");
}

extern "C" int eslam_tsdf_sample_color(const float* color, int64_t nx, int64_t ny, int64_t nz, const float* origin3_host,
                                       float voxel, const float* pts, int64_t n, float* out, eslam_stream_t stream) {
    TsdfGrid g;
    if (!tsdf_grid("eslam_tsdf_sample_color", nx, ny, nz, origin3_host, voxel, g)) return 1;
    if (n < 0 || n > (int64_t)0x7fffffff * TSDF_THREADS) {
        eslam_set_error("eslam_tsdf_sample_color: %lld points out of range", (long long)n);
        return 1;
    }
    if (n == 0) return 0;
    if (!color || !pts || !out) {
        eslam_set_error("eslam_tsdf_sample_color: null argument");
        return 1;
    }
    hipLaunchKernelGGL(tsdf_sample_color_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0,
                       (hipStream_t)stream, color, g, pts, n, out);
    return eslam_check_launch("tsdf_sample_color_kernel");
}
