// Frame preparation: the raw decoded RGB-D images (uint8 colour, uint16 depth) -> the float32 colour and depth images the
// tracking / mapping loop samples, i.e. what BaseDataset.__getitem__ (src/utils/datasets.py, reference datasets.py:88-114)
// computes on the host in float64, as one or two launches on the device.  The arithmetic is in include/eslam_hip.h
// (eslam_frame_*) and DESIGN.md section 18; tests/frame_ref.py mirrors it in numpy.
//
// The colour chain [undistort] -> [resize to the depth size] -> [resize to crop_size] -> [edge trim] -> / 255 is evaluated
// per OUTPUT pixel by nested taps: the trimmed pixel is a pixel of the crop_size image, whose (up to) 2 x 2 taps are pixels
// of the depth-sized image, each of which has (up to) 2 x 2 taps in the source bytes.  No intermediate float image exists.
// Undistortion rounds to uint8 on the host (cv2.undistort returns bytes), so it is a kernel of its own that writes a byte
// image for the chain to read.  Tap positions and weights are computed in float64 (the host resizes a float64 image, and a
// float32 coordinate near 1296 is 1e-4 of a pixel off); the blends are float32.  Built with -ffp-contract=off: the depth
// path and the undistortion are float32 operation by operation (a fused operation is written fmaf).
//
// A frame that needs none of the stages (Replica) takes the flat kernel: both images as byte / half-word streams, four
// elements per lane (one 4-byte or 8-byte load, one 16-byte store).
#include "eslam_common.h"

#define FRAME_THREADS 256
#define FRAME_MAX_DIM 16384

struct FramePlan {
    int Hc, Wc;        // colour image as decoded (after undistortion: same size)
    int Hd, Wd;        // depth image as decoded; the colour image is resized to it (stage 1)
    int H2, W2;        // crop_size, or (Hd, Wd) when there is none (stage 2)
    int edge;          // trimmed on every side of the stage-2 image
    int Ho, Wo;        // output
    float png_depth_scale, scale;
};

// ---- tap rules (torch's upsample index arithmetic, float64) -------------------------------------------------------
struct Tap {
    int i0, i1;
    float w0, w1;
};

// F.interpolate(mode='bilinear') along one axis of `in` samples resized to `out`: position dst of the output.
template <bool ALIGN>
__device__ __forceinline__ Tap bilinear_tap(int dst, int in, int out) {
    Tap t;
    if (in == out) {                     // (torch's own short cut; also what an absent stage is)
        t.i0 = t.i1 = dst;
        t.w0 = 1.0f;
        t.w1 = 0.0f;
        return t;
    }
    double src;
    if (ALIGN) {
        const double s = out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0;
        src = s * (double)dst;
    } else {
        const double s = (double)in / (double)out;
        src = s * ((double)dst + 0.5) - 0.5;
        if (src < 0.0) src = 0.0;
    }
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;        // (cannot happen for dst < out; keeps every index inside whatever dst is)
    const double l1 = src - (double)i0;
    t.i0 = i0;
    t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    t.w0 = (float)(1.0 - l1);
    t.w1 = (float)l1;
    return t;
}

// F.interpolate(mode='nearest') of a float32 image: float32 scale, floorf, clamped
__device__ __forceinline__ int nearest_index(int dst, int in, int out) {
    if (in == out) return dst;
    const float s = (float)in / (float)out;
    int i = (int)floorf((float)dst * s);
    return i < in - 1 ? i : in - 1;
}

__device__ __forceinline__ float depth_value(uint16_t raw, float png_depth_scale, float scale) {
    return ((float)raw / png_depth_scale) * scale;
}

// ---- the chain, one output pixel per lane ---------------------------------------------------------------------------
// one pixel (3 channels) of the depth-sized image: the stage-1 blend of the source bytes, values in [0, 255]
__device__ __forceinline__ void stage1_pixel(const uint8_t* __restrict__ rgb, const FramePlan& p, int y, int x, float out[3]) {
    const Tap ty = bilinear_tap<false>(y, p.Hc, p.Hd), tx = bilinear_tap<false>(x, p.Wc, p.Wd);
    const uint8_t* r0 = rgb + ((int64_t)ty.i0 * p.Wc) * 3;
    const uint8_t* r1 = rgb + ((int64_t)ty.i1 * p.Wc) * 3;
    if (tx.w1 == 0.0f && ty.w1 == 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (float)r0[tx.i0 * 3 + c];
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = tx.w0 * (float)r0[tx.i0 * 3 + c] + tx.w1 * (float)r0[tx.i1 * 3 + c];
        const float b = tx.w0 * (float)r1[tx.i0 * 3 + c] + tx.w1 * (float)r1[tx.i1 * 3 + c];
        out[c] = ty.w0 * a + ty.w1 * b;
    }
}

__global__ __launch_bounds__(FRAME_THREADS) void frame_chain_kernel(const uint8_t* __restrict__ rgb,
                                                                    const uint16_t* __restrict__ depth, const FramePlan p,
                                                                    float* __restrict__ color_out,
                                                                    float* __restrict__ depth_out) {
    const int64_t i = (int64_t)blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (i >= (int64_t)p.Ho * p.Wo) return;
    const int oy = (int)(i / p.Wo), ox = (int)(i - (int64_t)oy * p.Wo);
    const int y2 = oy + p.edge, x2 = ox + p.edge;                   // pixel of the stage-2 (crop_size) image
    // depth: nearest pixel of the decoded image
    const int dy = nearest_index(y2, p.Hd, p.H2), dx = nearest_index(x2, p.Wd, p.W2);
    depth_out[i] = depth_value(depth[(int64_t)dy * p.Wd + dx], p.png_depth_scale, p.scale);
    // colour: stage-2 taps (aligned corners) over stage-1 pixels
    const Tap ty = bilinear_tap<true>(y2, p.Hd, p.H2), tx = bilinear_tap<true>(x2, p.Wd, p.W2);
    float v[3];
    if (tx.w1 == 0.0f && ty.w1 == 0.0f) {
        stage1_pixel(rgb, p, ty.i0, tx.i0, v);
    } else {
        float a0[3], a1[3], b0[3], b1[3];
        stage1_pixel(rgb, p, ty.i0, tx.i0, a0);
        stage1_pixel(rgb, p, ty.i0, tx.i1, a1);
        stage1_pixel(rgb, p, ty.i1, tx.i0, b0);
        stage1_pixel(rgb, p, ty.i1, tx.i1, b1);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ty.w0 * (tx.w0 * a0[c] + tx.w1 * a1[c]) + ty.w1 * (tx.w0 * b0[c] + tx.w1 * b1[c]);
    }
    float* o = color_out + i * 3;
    o[0] = v[0] / 255.0f;
    o[1] = v[1] / 255.0f;
    o[2] = v[2] / 255.0f;
}

// ---- no stage at all: flat streams, four elements per lane ---------------------------------------------------------
// lanes [0, nq_c) take four colour bytes each, lanes [nq_c, nq_c + nq_d) four depth samples; the (< 4) elements left over
// at the end of either stream go to the last lanes one by one
__global__ __launch_bounds__(FRAME_THREADS) void frame_flat_kernel(const uint8_t* __restrict__ rgb, int64_t n_c,
                                                                   const uint16_t* __restrict__ depth, int64_t n_d,
                                                                   float png_depth_scale, float scale,
                                                                   float* __restrict__ color_out,
                                                                   float* __restrict__ depth_out) {
    const int64_t nq_c = n_c >> 2, nq_d = n_d >> 2;
    int64_t i = (int64_t)blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (i < nq_c) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(rgb)[i];
        float4_t o;
        o.x = (float)(w & 0xffu) / 255.0f;
        o.y = (float)((w >> 8) & 0xffu) / 255.0f;
        o.z = (float)((w >> 16) & 0xffu) / 255.0f;
        o.w = (float)(w >> 24) / 255.0f;
        reinterpret_cast<float4_t*>(color_out)[i] = o;
        return;
    }
    i -= nq_c;
    if (i < nq_d) {
        const uint2 w = reinterpret_cast<const uint2*>(depth)[i];
        float4_t o;
        o.x = depth_value((uint16_t)(w.x & 0xffffu), png_depth_scale, scale);
        o.y = depth_value((uint16_t)(w.x >> 16), png_depth_scale, scale);
        o.z = depth_value((uint16_t)(w.y & 0xffffu), png_depth_scale, scale);
        o.w = depth_value((uint16_t)(w.y >> 16), png_depth_scale, scale);
        reinterpret_cast<float4_t*>(depth_out)[i] = o;
        return;
    }
    i -= nq_d;
    const int64_t tail_c = n_c - (nq_c << 2), tail_d = n_d - (nq_d << 2);
    if (i < tail_c) {
        const int64_t k = (nq_c << 2) + i;
        color_out[k] = (float)rgb[k] / 255.0f;
    } else if (i - tail_c < tail_d) {
        const int64_t k = (nq_d << 2) + (i - tail_c);
        depth_out[k] = depth_value(depth[k], png_depth_scale, scale);
    }
}

// ---- undistortion: F.grid_sample(bilinear, zeros, align_corners=True) of the byte image, rounded back to bytes --------
// grid [H][W][2] float32 in [-1, 1] coordinates (x, y), as datasets.undistort_map builds it.  float32 throughout, in the
// order of torch's CPU kernel: pixel = (g + 1) * ((size - 1) / 2); the four weights e s, w s, e n, w n from the fractions;
// the sum nw, then ne, sw, se each added with one fused multiply-add; taps outside the image count as 0.
__global__ __launch_bounds__(FRAME_THREADS) void frame_undistort_kernel(const uint8_t* __restrict__ rgb,
                                                                        const float* __restrict__ grid, int H, int W,
                                                                        uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const float2 g = reinterpret_cast<const float2*>(grid)[i];
    const float x = (g.x + 1.0f) * ((float)(W - 1) / 2.0f);
    const float y = (g.y + 1.0f) * ((float)(H - 1) / 2.0f);
    const float xf = floorf(x), yf = floorf(y);
    const float w = x - xf, e = 1.0f - w, n = y - yf, s = 1.0f - n;
    const float wt[4] = {e * s, w * s, e * n, w * n};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    // (a NaN or a far-away coordinate fails every range test below: the pixel is 0)
    const bool fin = xf >= -2.0f && xf <= (float)W && yf >= -2.0f && yf <= (float)H;
    const int x0 = fin ? (int)xf : -2, y0 = fin ? (int)yf : -2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        const bool in = xx >= 0 && xx < W && yy >= 0 && yy < H;
        const uint8_t* q = rgb + ((int64_t)(in ? yy : 0) * W + (in ? xx : 0)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = in ? (float)q[c] : 0.0f;
            acc[c] = k == 0 ? v * wt[0] : fmaf(v, wt[k], acc[c]);
        }
    }
    uint8_t* o = out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float r = fminf(fmaxf(rintf(acc[c]), 0.0f), 255.0f);        // round half to even, as torch.round
        o[c] = (uint8_t)(r == r ? (int)r : 0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool frame_dim_ok(int v) { return v >= 1 && v <= FRAME_MAX_DIM; }

// validates the geometry and fills the plan; pure host arithmetic
static bool frame_plan(const char* who, int Hc, int Wc, int Hd, int Wd, int crop_h, int crop_w, int edge, FramePlan& p) {
    if (!frame_dim_ok(Hc) || !frame_dim_ok(Wc) || !frame_dim_ok(Hd) || !frame_dim_ok(Wd)) {
        eslam_set_error("%s: image sizes %d x %d (colour) and %d x %d (depth) must lie in [1, %d]", who, Wc, Hc, Wd, Hd, FRAME_MAX_DIM);
        return false;
    }
    if ((crop_h == 0) != (crop_w == 0) || crop_h < 0 || crop_w < 0 || crop_h > FRAME_MAX_DIM || crop_w > FRAME_MAX_DIM) {
        eslam_set_error("%s: crop_size %d x %d: both 0 (none) or both in [1, %d]", who, crop_w, crop_h, FRAME_MAX_DIM);
        return false;
    }
    p.Hc = Hc; p.Wc = Wc; p.Hd = Hd; p.Wd = Wd;
    p.H2 = crop_h ? crop_h : Hd;
    p.W2 = crop_w ? crop_w : Wd;
    if (edge < 0 || 2 * (int64_t)edge >= p.H2 || 2 * (int64_t)edge >= p.W2) {
        eslam_set_error("%s: crop_edge %d leaves nothing of a %d x %d image", who, edge, p.W2, p.H2);
        return false;
    }
    p.edge = edge;
    p.Ho = p.H2 - 2 * edge;
    p.Wo = p.W2 - 2 * edge;
    return true;
}

extern "C" int eslam_frame_out_shape(int Hc, int Wc, int Hd, int Wd, int crop_h, int crop_w, int crop_edge, int* H_out_host,
                                     int* W_out_host) {
    FramePlan p;
    if (!frame_plan("eslam_frame_out_shape", Hc, Wc, Hd, Wd, crop_h, crop_w, crop_edge, p)) return 1;
    if (!H_out_host || !W_out_host) {
        eslam_set_error("eslam_frame_out_shape: null argument");
        return 1;
    }
    *H_out_host = p.Ho;
    *W_out_host = p.Wo;
    return 0;
}

extern "C" int eslam_frame_undistort(const uint8_t* rgb, const float* grid, int H, int W, uint8_t* out, eslam_stream_t stream) {
    if (!frame_dim_ok(H) || !frame_dim_ok(W)) {
        eslam_set_error("eslam_frame_undistort: image size %d x %d must lie in [1, %d]", W, H, FRAME_MAX_DIM);
        return 1;
    }
    if (!rgb || !grid || !out || rgb == out) {
        eslam_set_error("eslam_frame_undistort: null argument, or the output is the input");
        return 1;
    }
    if ((uintptr_t)grid % 8 != 0) {
        eslam_set_error("eslam_frame_undistort: the grid must be 8-byte aligned");
        return 1;
    }
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(frame_undistort_kernel, dim3((unsigned)((n + FRAME_THREADS - 1) / FRAME_THREADS)), dim3(FRAME_THREADS), 0,
                       (hipStream_t)stream, rgb, grid, H, W, out);
    return eslam_check_launch("frame_undistort_kernel");
}

extern "C" int eslam_frame_prepare(const uint8_t* rgb, int Hc, int Wc, const uint16_t* depth, int Hd, int Wd, int crop_h,
                                   int crop_w, int crop_edge, float png_depth_scale, float scale, float* color_out,
                                   float* depth_out, eslam_stream_t stream) {
    FramePlan p;
    if (!frame_plan("eslam_frame_prepare", Hc, Wc, Hd, Wd, crop_h, crop_w, crop_edge, p)) return 1;
    if (!(png_depth_scale > 0.0f) || !(scale == scale)) {
        eslam_set_error("eslam_frame_prepare: png_depth_scale %g must be positive and scale %g a number", (double)png_depth_scale,
                        (double)scale);
        return 1;
    }
    if (!rgb || !depth || !color_out || !depth_out) {
        eslam_set_error("eslam_frame_prepare: null argument");
        return 1;
    }
    if ((uintptr_t)depth % 2 != 0 || (uintptr_t)color_out % 4 != 0 || (uintptr_t)depth_out % 4 != 0) {
        eslam_set_error("eslam_frame_prepare: misaligned depth image or output");
        return 1;
    }
    p.png_depth_scale = png_depth_scale;
    p.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    const bool identity = Hc == Hd && Wc == Wd && p.H2 == Hd && p.W2 == Wd && crop_edge == 0;
    const bool wide_ok = (uintptr_t)rgb % 4 == 0 && (uintptr_t)depth % 8 == 0 && (uintptr_t)color_out % 16 == 0 &&
                         (uintptr_t)depth_out % 16 == 0;
    if (identity && wide_ok) {
        const int64_t n_d = (int64_t)Hd * Wd, n_c = n_d * 3;
        const int64_t lanes = (n_c >> 2) + (n_d >> 2) + (n_c & 3) + (n_d & 3);
        hipLaunchKernelGGL(frame_flat_kernel, dim3((unsigned)((lanes + FRAME_THREADS - 1) / FRAME_THREADS)), dim3(FRAME_THREADS), 0,
                           st, rgb, n_c, depth, n_d, png_depth_scale, scale, color_out, depth_out);
        return eslam_check_launch("frame_flat_kernel");
    }
    const int64_t n = (int64_t)p.Ho * p.Wo;
    hipLaunchKernelGGL(frame_chain_kernel, dim3((unsigned)((n + FRAME_THREADS - 1) / FRAME_THREADS)), dim3(FRAME_THREADS), 0, st,
                       rgb, depth, p, color_out, depth_out);
    return eslam_check_launch("frame_chain_kernel");
}
