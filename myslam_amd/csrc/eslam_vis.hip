// Frame visualiser panels and render metrics: three operations on a rendered frame (depth [H][W], colour [H][W][3]) and its
// ground truth, all float32 on the device.  The definitions are in include/eslam_hip.h (eslam_frame_stats, eslam_ssim,
// eslam_vis_panel) and DESIGN.md section 19; tests/vis_ref.py mirrors them in numpy.
//
//   frame_stats   masked sums and the maximum, a two-stage fixed-order float64 tree (no float atomics)
//   ssim          mean SSIM with the 11 x 11 Gaussian window over the valid region: one output tile per workgroup, the
//                 tile and its 10-pixel halo of both images staged in LDS, the horizontal pass of the five moment images
//                 into LDS, the vertical pass and the formula in registers
//   vis_panel     the 2 x 3 panel of Frame_Visualizer as bytes: plasma-mapped depths, clipped colours, masked residuals
//
// Built with -ffp-contract=off: the panel is compared bit for bit with a float32 numpy model, and the SSIM's operation
// order (below, and in the header) is the one the float32 model follows.
#include "eslam_common.h"

#define VIS_THREADS 256
#define VIS_MAX_DIM 16384
#define STATS_PIXELS ESLAM_STATS_BLOCK_PIXELS        // pixels per workgroup of the first stage: 16 per thread
#define SSIM_TH ESLAM_SSIM_TILE_H
#define SSIM_TW ESLAM_SSIM_TILE_W
#define SSIM_WIN 11
#define SSIM_IH (SSIM_TH + SSIM_WIN - 1)             // staged rows
#define SSIM_IW (SSIM_TW + SSIM_WIN - 1)             // staged columns

static_assert(STATS_PIXELS % VIS_THREADS == 0, "a thread takes a whole number of pixels");
static_assert((SSIM_TH * SSIM_TW) % VIS_THREADS == 0, "a thread takes a whole number of output pixels");

// sum of one double per thread over the workgroup, in a fixed order; every thread gets the result
__device__ __forceinline__ double vis_tree_sum(double* lds, double v) {
    __syncthreads();                                 // (the array may still be read by the previous tree)
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = VIS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

__device__ __forceinline__ double vis_tree_max(double* lds, double v) {
    __syncthreads();
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = VIS_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] = fmax(lds[threadIdx.x], lds[threadIdx.x + s]);
        __syncthreads();
    }
    return lds[0];
}

// ---------------------------------------------------------------------------------------------------------
// frame stats
// ---------------------------------------------------------------------------------------------------------
// workgroup b takes the pixels [b STATS_PIXELS, (b + 1) STATS_PIXELS) and the colour values of those pixels as one flat run;
// thread t every 256th element from t.  partial [n_blocks][4]
__global__ __launch_bounds__(VIS_THREADS) void frame_stats_partial_kernel(const float* __restrict__ depth,
                                                                          const float* __restrict__ gt_depth,
                                                                          const float* __restrict__ color,
                                                                          const float* __restrict__ gt_color, int64_t npix,
                                                                          double* __restrict__ partial) {
    __shared__ double lds[VIS_THREADS];
    const int64_t p0 = (int64_t)blockIdx.x * STATS_PIXELS, p1 = min(p0 + STATS_PIXELS, npix);
    double n_valid = 0.0, s_abs = 0.0, s_sq = 0.0, mx = -INFINITY;
    for (int64_t i = p0 + threadIdx.x; i < p1; i += VIS_THREADS) {
        const float g = gt_depth[i];
        if (g > 0.0f) {
            n_valid += 1.0;
            s_abs += (double)fabsf(depth[i] - g);
        }
        mx = fmax(mx, (double)g);
    }
    for (int64_t i = 3 * p0 + threadIdx.x; i < 3 * p1; i += VIS_THREADS) {
        const double d = (double)(color[i] - gt_color[i]);
        s_sq += d * d;
    }
    n_valid = vis_tree_sum(lds, n_valid);
    s_abs = vis_tree_sum(lds, s_abs);
    s_sq = vis_tree_sum(lds, s_sq);
    mx = vis_tree_max(lds, mx);
    if (threadIdx.x == 0) {
        double* o = partial + (int64_t)blockIdx.x * 4;
        o[0] = n_valid;
        o[1] = s_abs;
        o[2] = s_sq;
        o[3] = mx;
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then the tree
__global__ __launch_bounds__(VIS_THREADS) void frame_stats_final_kernel(const double* __restrict__ partial, int n_blocks,
                                                                        double* __restrict__ out) {
    __shared__ double lds[VIS_THREADS];
    double n_valid = 0.0, s_abs = 0.0, s_sq = 0.0, mx = -INFINITY;
    for (int b = threadIdx.x; b < n_blocks; b += VIS_THREADS) {
        const double* p = partial + (int64_t)b * 4;
        n_valid += p[0];
        s_abs += p[1];
        s_sq += p[2];
        mx = fmax(mx, p[3]);
    }
    n_valid = vis_tree_sum(lds, n_valid);
    s_abs = vis_tree_sum(lds, s_abs);
    s_sq = vis_tree_sum(lds, s_sq);
    mx = vis_tree_max(lds, mx);
    if (threadIdx.x == 0) {
        out[0] = n_valid;
        out[1] = s_abs;
        out[2] = s_sq;
        out[3] = mx;
    }
}

// ---------------------------------------------------------------------------------------------------------
// SSIM
// ---------------------------------------------------------------------------------------------------------
struct SsimWindow {
    float w[SSIM_WIN];
};

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// Workgroup (bx, by, c): the outputs [by TH, by TH + TH) x [bx TW, bx TW + TW) of channel c, cut at the map's edge.
// Operation order (float32, no contraction; w = the window's weights, sums run k = 0 .. 10 as acc = w[0] v[0], then
// acc = acc + w[k] v[k]):
//   kx, ky          the clipped values of a and b at the tile's first pixel (row by TH, column bx TW, channel c)
//   x = clip(a) - kx,  y = clip(b) - ky                                       staged
//   h_x, h_y, h_xx, h_yy, h_xy  = sum_k w[k] {x, y, x x, y y, x y}[r][j + k]    horizontal pass
//   m_* = sum_k w[k] h_*[i + k][j]                                            vertical pass
//   vx = m_xx - m_x m_x,  vy = m_yy - m_y m_y,  vxy = m_xy - m_x m_y          (moments of the shifted values)
//   ux = kx + m_x,  uy = ky + m_y
//   ssim = ((2 (ux uy) + C1) (2 vxy + C2)) / ((ux ux + uy uy + C1) (vx + vy + C2))
__global__ __launch_bounds__(VIS_THREADS) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                                int W, int C, const SsimWindow win, float* __restrict__ map,
                                                                double* __restrict__ partial) {
    __shared__ float xs[SSIM_IH][SSIM_IW], ys[SSIM_IH][SSIM_IW];
    __shared__ float hz[5][SSIM_IH][SSIM_TW];
    __shared__ double red[VIS_THREADS];
    const int tid = threadIdx.x, c = blockIdx.z;
    const int Ho = H - (SSIM_WIN - 1), Wo = W - (SSIM_WIN - 1);
    const int y0 = blockIdx.y * SSIM_TH, x0 = blockIdx.x * SSIM_TW;
    const int th = min(SSIM_TH, Ho - y0), tw = min(SSIM_TW, Wo - x0);          // this tile's outputs (>= 1 each)
    const int ih = th + SSIM_WIN - 1, iw = tw + SSIM_WIN - 1;                  // its input rows and columns, inside the image
    const int64_t origin = ((int64_t)y0 * W + x0) * C + c;
    const float kx = clip01(a[origin]), ky = clip01(b[origin]);

    for (int p = tid; p < SSIM_IH * SSIM_IW; p += VIS_THREADS) {
        const int r = p / SSIM_IW, q = p - r * SSIM_IW;
        float x = 0.0f, y = 0.0f;
        if (r < ih && q < iw) {
            const int64_t at = origin + ((int64_t)r * W + q) * C;
            x = clip01(a[at]) - kx;
            y = clip01(b[at]) - ky;
        }
        xs[r][q] = x;
        ys[r][q] = y;
    }
    __syncthreads();

    for (int p = tid; p < SSIM_IH * SSIM_TW; p += VIS_THREADS) {
        const int r = p / SSIM_TW, j = p - r * SSIM_TW;
        float hx, hy, hxx, hyy, hxy;
        {
            const float x = xs[r][j], y = ys[r][j], w = win.w[0];
            hx = w * x;
            hy = w * y;
            hxx = w * (x * x);
            hyy = w * (y * y);
            hxy = w * (x * y);
        }
#pragma unroll
        for (int k = 1; k < SSIM_WIN; ++k) {
            const float x = xs[r][j + k], y = ys[r][j + k], w = win.w[k];
            hx = hx + w * x;
            hy = hy + w * y;
            hxx = hxx + w * (x * x);
            hyy = hyy + w * (y * y);
            hxy = hxy + w * (x * y);
        }
        hz[0][r][j] = hx;
        hz[1][r][j] = hy;
        hz[2][r][j] = hxx;
        hz[3][r][j] = hyy;
        hz[4][r][j] = hxy;
    }
    __syncthreads();

    const float C1 = 1e-4f, C2 = 9e-4f;
    double acc = 0.0;
    for (int p = tid; p < SSIM_TH * SSIM_TW; p += VIS_THREADS) {
        const int i = p / SSIM_TW, j = p - i * SSIM_TW;
        float m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = win.w[0] * hz[q][i][j];
#pragma unroll
        for (int k = 1; k < SSIM_WIN; ++k) {
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = m[q] + win.w[k] * hz[q][i + k][j];
        }
        const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], vxy = m[4] - m[0] * m[1];
        const float ux = kx + m[0], uy = ky + m[1];
        const float num = (2.0f * (ux * uy) + C1) * (2.0f * vxy + C2);
        const float den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
        const float s = num / den;
        if (i < th && j < tw) {
            if (map) map[((int64_t)(y0 + i) * Wo + (x0 + j)) * C + c] = s;
            acc += (double)s;
        }
    }
    const double total = vis_tree_sum(red, acc);
    if (tid == 0) partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(VIS_THREADS) void ssim_final_kernel(const double* __restrict__ partial, int n_blocks, double count,
                                                                 double* __restrict__ mean) {
    __shared__ double lds[VIS_THREADS];
    double s = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += VIS_THREADS) s += partial[b];
    s = vis_tree_sum(lds, s);
    if (threadIdx.x == 0) mean[0] = s / count;
}

// ---------------------------------------------------------------------------------------------------------
// the panel
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int plasma_index(float v, float vmax) {
    const float t = v / vmax;
    if (!(t > 0.0f)) return 0;                       // t <= 0 or NaN
    return t >= 1.0f ? 255 : (int)(t * 256.0f);      // = min(255, int(t 256)): t 256 is exact, and below 256 when t < 1
}

__device__ __forceinline__ uint8_t color_byte(float c) { return (uint8_t)(int)(clip01(c) * 255.0f + 0.5f); }

// one output pixel per thread
__global__ __launch_bounds__(VIS_THREADS) void vis_panel_kernel(const float* __restrict__ depth, const float* __restrict__ gt_depth,
                                                                const float* __restrict__ color,
                                                                const float* __restrict__ gt_color, int H, int W,
                                                                const double* __restrict__ stats, const uint8_t* __restrict__ lut,
                                                                uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * VIS_THREADS + threadIdx.x;
    const int64_t PW = 3 * (int64_t)W;
    if (i >= 2 * (int64_t)H * PW) return;
    const int py = (int)(i / PW), px = (int)(i - (int64_t)py * PW);
    const int row = py >= H, col = px / W;
    const int y = py - row * H, x = px - col * W;
    const int64_t at = (int64_t)y * W + x;
    const float g = gt_depth[at];
    uint8_t* o = out + i * 3;
    if (row == 0) {
        float vmax = (float)stats[3];
        if (vmax == 0.0f) vmax = 1.0f;
        float v = g;
        if (col == 1) v = depth[at];
        if (col == 2) v = g == 0.0f ? 0.0f : fabsf(g - depth[at]);
        const uint8_t* e = lut + 3 * plasma_index(v, vmax);
        o[0] = e[0];
        o[1] = e[1];
        o[2] = e[2];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = gt_color[at * 3 + c];
            if (col == 1) v = color[at * 3 + c];
            if (col == 2) v = g == 0.0f ? 0.0f : fabsf(v - color[at * 3 + c]);
            o[c] = color_byte(v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool vis_dim_ok(int v) { return v >= 1 && v <= VIS_MAX_DIM; }

static int64_t stats_blocks(int H, int W) { return ((int64_t)H * W + STATS_PIXELS - 1) / STATS_PIXELS; }

extern "C" int64_t eslam_frame_stats_workspace_bytes(int H, int W) {
    return vis_dim_ok(H) && vis_dim_ok(W) ? stats_blocks(H, W) * 4 * 8 : -1;
}

extern "C" int eslam_frame_stats(const float* depth, const float* gt_depth, const float* color, const float* gt_color, int H,
                                 int W, void* workspace, double* out, eslam_stream_t stream) {
    if (!vis_dim_ok(H) || !vis_dim_ok(W)) {
        eslam_set_error("eslam_frame_stats: image size %d x %d must lie in [1, %d]", W, H, VIS_MAX_DIM);
        return 1;
    }
    if (!depth || !gt_depth || !color || !gt_color || !workspace || !out) {
        eslam_set_error("eslam_frame_stats: null argument");
        return 1;
    }
    const int n_blocks = (int)stats_blocks(H, W);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(frame_stats_partial_kernel, dim3(n_blocks), dim3(VIS_THREADS), 0, st, depth, gt_depth, color, gt_color,
                       (int64_t)H * W, partial);
    if (eslam_check_launch("frame_stats_partial_kernel")) return 1;
    hipLaunchKernelGGL(frame_stats_final_kernel, dim3(1), dim3(VIS_THREADS), 0, st, partial, n_blocks, out);
    return eslam_check_launch("frame_stats_final_kernel");
}

static bool ssim_shape_ok(const char* who, int H, int W, int C) {
    if (H < SSIM_WIN || W < SSIM_WIN || H > VIS_MAX_DIM || W > VIS_MAX_DIM) {
        eslam_set_error("%s: image size %d x %d must lie in [%d, %d] (the window is %d x %d, no padding)", who, W, H, SSIM_WIN,
                        VIS_MAX_DIM, SSIM_WIN, SSIM_WIN);
        return false;
    }
    if (C != 1 && C != 3) {
        eslam_set_error("%s: %d channels; 1 or 3 are built", who, C);
        return false;
    }
    return true;
}

static void ssim_grid(int H, int W, int& gx, int& gy) {
    gx = (W - (SSIM_WIN - 1) + SSIM_TW - 1) / SSIM_TW;
    gy = (H - (SSIM_WIN - 1) + SSIM_TH - 1) / SSIM_TH;
}

extern "C" int64_t eslam_ssim_workspace_bytes(int H, int W, int C) {
    if (!ssim_shape_ok("eslam_ssim_workspace_bytes", H, W, C)) return -1;
    int gx, gy;
    ssim_grid(H, W, gx, gy);
    return (int64_t)gx * gy * C * 8;
}

extern "C" int eslam_ssim(const float* a, const float* b, int H, int W, int C, void* workspace, float* map, double* mean,
                          eslam_stream_t stream) {
    if (!ssim_shape_ok("eslam_ssim", H, W, C)) return 1;
    if (!a || !b || !workspace || !mean) {
        eslam_set_error("eslam_ssim: null argument");
        return 1;
    }
    // the window: exp(-(k - 5)^2 / (2 sigma^2)), normalised in float64, rounded to float32
    SsimWindow win;
    double g[SSIM_WIN], sum = 0.0;
    for (int k = 0; k < SSIM_WIN; ++k) {
        const double d = (double)(k - SSIM_WIN / 2);
        g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < SSIM_WIN; ++k) win.w[k] = (float)(g[k] / sum);
    int gx, gy;
    ssim_grid(H, W, gx, gy);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3(gx, gy, C), dim3(VIS_THREADS), 0, st, a, b, H, W, C, win, map, partial);
    if (eslam_check_launch("ssim_tile_kernel")) return 1;
    const double count = (double)(H - (SSIM_WIN - 1)) * (double)(W - (SSIM_WIN - 1)) * (double)C;
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(VIS_THREADS), 0, st, partial, gx * gy * C, count, mean);
    return eslam_check_launch("ssim_final_kernel");
}

extern "C" int eslam_vis_panel(const float* depth, const float* gt_depth, const float* color, const float* gt_color, int H, int W,
                               const double* stats, const uint8_t* lut, uint8_t* out, eslam_stream_t stream) {
    if (!vis_dim_ok(H) || !vis_dim_ok(W)) {
        eslam_set_error("eslam_vis_panel: image size %d x %d must lie in [1, %d]", W, H, VIS_MAX_DIM);
        return 1;
    }
    if (!depth || !gt_depth || !color || !gt_color || !stats || !lut || !out) {
        eslam_set_error("eslam_vis_panel: null argument");
        return 1;
    }
    const int64_t n = 6 * (int64_t)H * W;
    hipLaunchKernelGGL(vis_panel_kernel, dim3((unsigned)((n + VIS_THREADS - 1) / VIS_THREADS)), dim3(VIS_THREADS), 0,
                       (hipStream_t)stream, depth, gt_depth, color, gt_color, H, W, stats, lut, out);
    return eslam_check_launch("vis_panel_kernel");
}
