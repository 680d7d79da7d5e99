// eslam_sdf_grad: the SDF and its gradient with respect to the point, in one launch, nothing per point in HBM but
// 12 bytes in and 16 bytes out.  The tile is decode_fwd_kernel's on its PointList source (eslam_decode_tile.h: 64 points
// per wave in 4 blocks of 16, gather role -> MFMA role -> sample role), run in FORWARD mode: while the eight 16-byte taps
// of a plane are in registers the lane accumulates, beside the 8 channel values, their derivatives along the plane's two
// axes (coord_grad8's su / sv per channel, eslam_render_bwd.hip, with ATen's border gate and the (n - 1) / 2 factor) into
// three tangent vectors d feat / d x, d y, d z.  Value and tangents then go through the SDF decoder with the same DecFrag:
// a tangent's layers are plain MFMA products without bias, masked by the sign of the value's pre-activation, and the output
// layer places all four results in the sample role as mlp_out_accum does.  Texels are loaded once; no transposed weights.
//
// The value path is decode_fwd_kernel<CL, SDF_ONLY>'s to the operation, so that sdf is bit-identical.  One step needs care:
// accumulate_taps / gather8 write a texel's bilinear sum as a00 w00 + a01 w01 + a10 w10 + a11 w11 and leave its contraction
// into FMAs to the compiler, which in the decode kernels settles on  acc + fma(a11, w11, fma(a10, w10, fma(a00, w00, a01 w01)))
// for every channel of every plane, but beside the tangent arithmetic of this kernel vectorises some channels differently
// and leaves their products unfused (a last-bit difference in about 1 sdf of 200).  bilerp_as_decode spells that form out.
// The NCHW decode kernel (gather8<false>) has one exception of its own, which bilerp_as_decode_nchw_tail spells out as well:
// on the fine xy plane its last two channels of a piece (i = 6, 7) come out as ((fma(a00, w00, a01 w01) + a10 w10) + a11 w11),
// the last two products unfused.  tests/test_gpu_sdf_normals.py holds both layouts to decode_sdf_only bit for bit, so a
// compiler that contracts the decode kernels differently shows there.
#include "eslam_decode_tile.h"

struct GeoPlaneSet {                     // the six geometry planes: xy, xz, yz x (coarse, fine), index 2 * o + lvl
    eslam_plane_t p[6];
};

struct TapGeom {                         // per plane and lane: the bilinear fractions and d(ix)/du, d(iy)/dv
    float tx, ty;
    float su, sv;                        // (n - 1) / 2 strictly inside, 0 where the border clamp is active
};

__device__ __forceinline__ void tap_geom(const eslam_plane_t& P, float u, float v, TapGeom& g) {
    const AxisCoord ax = axis_coord(u, P.w);
    const AxisCoord ay = axis_coord(v, P.h);
    g.tx = ax.t;
    g.ty = ay.t;
    g.su = ax.inside ? 0.5f * (float)(P.w - 1) : 0.0f;
    g.sv = ay.inside ? 0.5f * (float)(P.h - 1) : 0.0f;
}

__device__ __forceinline__ float bilerp_as_decode(float t00, float t01, float t10, float t11, float w00, float w01, float w10,
                                                  float w11) {
    return __builtin_fmaf(t11, w11, __builtin_fmaf(t10, w10, __builtin_fmaf(t00, w00, t01 * w01)));
}

__device__ __forceinline__ float bilerp_as_decode_nchw_tail(float t00, float t01, float t10, float t11, float w00, float w01,
                                                            float w10, float w11) {
#pragma clang fp contract(off)
    float m = __builtin_fmaf(t00, w00, t01 * w01);
    const float p10 = t10 * w10, p11 = t11 * w11;
    m = m + p10;
    m = m + p11;
    return m;
}

__device__ __forceinline__ void accumulate_taps_as_decode(const PlaneTaps& t, float acc[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[i] = acc[i] + bilerp_as_decode(t.a00[i], t.a01[i], t.a10[i], t.a11[i], t.w00, t.w01, t.w10, t.w11);
        acc[4 + i] = acc[4 + i] + bilerp_as_decode(t.b00[i], t.b01[i], t.b10[i], t.b11[i], t.w00, t.w01, t.w10, t.w11);
    }
}

// derivative of one bilinear tap along u and v, scaled and gated, added to the tangents of those two axes
__device__ __forceinline__ void tangent1(float t00, float t01, float t10, float t11, const TapGeom& g, float& tu, float& tv) {
    tu += ((t01 - t00) * (1.0f - g.ty) + (t11 - t10) * g.ty) * g.su;
    tv += ((t10 - t00) * (1.0f - g.tx) + (t11 - t01) * g.tx) * g.sv;
}

__device__ __forceinline__ void accumulate_tangents(const PlaneTaps& t, const TapGeom& g, float tu[8], float tv[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tangent1(t.a00[i], t.a01[i], t.a10[i], t.a11[i], g, tu[i], tv[i]);
        tangent1(t.b00[i], t.b01[i], t.b10[i], t.b11[i], g, tu[4 + i], tv[4 + i]);
    }
}

// the reference's NCHW planes: one channel plane per load (gather role = MFMA role); values as gather8<false>
__device__ __forceinline__ void gather8_tangents_nchw(const bool fine_xy, const eslam_plane_t& P, float u, float v, int q, const TapGeom& g, float acc[8],
                                                      float tu[8], float tv[8]) {
    const AxisCoord ax = axis_coord(u, P.w);
    const AxisCoord ay = axis_coord(v, P.h);
    const float w00 = (1.0f - ax.t) * (1.0f - ay.t);
    const float w01 = ax.t * (1.0f - ay.t);
    const float w10 = (1.0f - ax.t) * ay.t;
    const float w11 = ax.t * ay.t;
    const unsigned sy = (unsigned)P.stride_y, sx = (unsigned)P.stride_x, sc = (unsigned)P.stride_c;
    const unsigned r0 = ay.i0 * sy, r1 = ay.i1 * sy, c0 = ax.i0 * sx, c1 = ax.i1 * sx;
    const float* __restrict__ data = P.data;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned co = (unsigned)piece_channel(q, i) * sc;
        const float t00 = data[co + r0 + c0], t01 = data[co + r0 + c1], t10 = data[co + r1 + c0], t11 = data[co + r1 + c1];
        acc[i] = acc[i] + (fine_xy && i >= 6 ? bilerp_as_decode_nchw_tail(t00, t01, t10, t11, w00, w01, w10, w11)
                                             : bilerp_as_decode(t00, t01, t10, t11, w00, w01, w10, w11));
        tangent1(t00, t01, t10, t11, g, tu[i], tv[i]);
    }
}

// value features and the three tangents of the lane's gather-role point; plane order and pipeline of gather_features
template <bool CL>
__device__ __forceinline__ void gather_features_tangents(const GeoPlaneSet& planes, float x, float y, float z, int q, float feat[16],
                                                         float fx[16], float fy[16], float fz[16], int opaque0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) feat[i] = fx[i] = fy[i] = fz[i] = 0.0f;
    if (CL) {
        PlaneTaps taps[2];
        TapGeom geom[2];
        issue_taps(planes.p[opaque0], ORIENT_U(0, x, y, z), ORIENT_V(0, x, y, z), q, taps[0]);
        tap_geom(planes.p[opaque0], ORIENT_U(0, x, y, z), ORIENT_V(0, x, y, z), geom[0]);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int kn = k + 1;
            if (kn < 6) {
                const eslam_plane_t& Pn = planes.p[2 * (kn % 3) + (kn / 3) + opaque0];
                issue_taps(Pn, ORIENT_U(kn % 3, x, y, z), ORIENT_V(kn % 3, x, y, z), q, taps[kn & 1]);
                tap_geom(Pn, ORIENT_U(kn % 3, x, y, z), ORIENT_V(kn % 3, x, y, z), geom[kn & 1]);
            }
            const int o = k % 3, lvl = k / 3;
            accumulate_taps_as_decode(taps[k & 1], feat + 8 * lvl);
            accumulate_tangents(taps[k & 1], geom[k & 1], (o == 2 ? fy : fx) + 8 * lvl, (o == 0 ? fy : fz) + 8 * lvl);
            __builtin_amdgcn_sched_barrier(0);
        }
        return;
    }
#pragma unroll
    for (int lvl = 0; lvl < 2; ++lvl) {
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const eslam_plane_t& P = planes.p[2 * o + lvl + opaque0];
            const float u = ORIENT_U(o, x, y, z), v = ORIENT_V(o, x, y, z);
            TapGeom g;
            tap_geom(P, u, v, g);
            gather8_tangents_nchw(lvl == 1 && o == 0, P, u, v, q, g, feat + 8 * lvl, (o == 2 ? fy : fx) + 8 * lvl, (o == 0 ? fy : fz) + 8 * lvl);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// one tangent through the decoder: W1 . t, masked by h1 > 0; W2 . that, masked by h2 > 0; the output row into `out`
__device__ __forceinline__ void mlp_tangent(const DecFrag& f, const float t[16], const float4_t& h1, const float4_t& h2, int b, int r,
                                            float4_t& out) {
    float4_t a1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) a1 = mfma16(f.w1[ks], t[ks], a1);
    float4_t a2 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a2 = mfma16(f.w2[ks], h1[ks] > 0.0f ? a1[ks] : 0.0f, a2);
    float4_t t2;
#pragma unroll
    for (int i = 0; i < 4; ++i) t2[i] = h2[i] > 0.0f ? a2[i] : 0.0f;
    mlp_out_accum(f, t2, b, r, out);
}

template <bool CL>
__global__ __launch_bounds__(256, 2) void sdf_grad_kernel(const GeoPlaneSet planes, const eslam_decoders_t dec, const Bound bnd,
                                                          const float* __restrict__ pts, const int64_t N, const int unit,
                                                          float* __restrict__ sdf_out, float* __restrict__ grad_out) {
    __shared__ __attribute__((aligned(16))) float wlds[DEC_LDS];
    stage_decoder_weights_one(wlds, dec, 0, threadIdx.x, blockDim.x);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;                                  // MFMA role
    const int gp = gather_point<CL>(lane), gq = gather_piece<CL>(lane);     // gather role
    const int64_t ntiles = (N + 63) / 64;
    const float sc3[3] = {2.0f / (bnd.hi[0] - bnd.lo[0]), 2.0f / (bnd.hi[1] - bnd.lo[1]), 2.0f / (bnd.hi[2] - bnd.lo[2])};

    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += (int64_t)gridDim.x * 4) {
        const int64_t p0 = t * 64;
        const int nvalid = (int)min((int64_t)64, N - p0);
        const int nblk = (nvalid + 15) >> 4;
        float4_t out = *(const float4_t*)(wlds + DEC_B3);
        float4_t ox = {0.0f, 0.0f, 0.0f, 0.0f}, oy = ox, oz = ox;
#pragma unroll 1
        for (int b = 0; b < nblk; ++b) {
            const int oz0 = opaque_zero(b);
            const float* p = pts + (p0 + min(16 * b + gp, nvalid - 1)) * 3;       // past the end: a clamped duplicate, never stored
            const float px = norm_coord(p[0], bnd.lo[0], bnd.hi[0]);
            const float py = norm_coord(p[1], bnd.lo[1], bnd.hi[1]);
            const float pz = norm_coord(p[2], bnd.lo[2], bnd.hi[2]);
            float feat[16], fx[16], fy[16], fz[16];
            gather_features_tangents<CL>(planes, px, py, pz, gq, feat, fx, fy, fz, oz0);
            to_mfma_role<CL, 16>(feat, lane);
            to_mfma_role<CL, 16>(fx, lane);
            to_mfma_role<CL, 16>(fy, lane);
            to_mfma_role<CL, 16>(fz, lane);
            DecFrag f;
            load_dec_frag(f, wlds + oz0, r, q);
            float4_t h1, h2;
            mlp_hidden(f, feat, h1, h2);
            mlp_out_accum(f, h2, b, r, out);
            mlp_tangent(f, fx, h1, h2, b, r, ox);
            mlp_tangent(f, fy, h1, h2, b, r, oy);
            mlp_tangent(f, fz, h1, h2, b, r, oz);
        }
        if (lane < nvalid) {             // sample role: lane l holds o, do/dx, do/dy, do/dz of point l (normalised coordinates)
            const float sdf = tanhf(out[0]);
            const float dt = 1.0f - sdf * sdf;
            float gx = ox[0] * dt * sc3[0], gy = oy[0] * dt * sc3[1], gz = oz[0] * dt * sc3[2];
            if (unit) {
                const float n2 = gx * gx + gy * gy + gz * gz;
                if (n2 == 0.0f) {
                    gx = gy = gz = 0.0f;
                } else {
                    const float n = sqrtf(n2);
                    gx /= n; gy /= n; gz /= n;
                }
            }
            if (sdf_out) sdf_out[p0 + lane] = sdf;
            float* g = grad_out + (p0 + lane) * 3;
            g[0] = gx; g[1] = gy; g[2] = gz;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
bool eslam_planes_channels_last(const eslam_plane_t* planes, int first, int count);
int eslam_validate_planes(const eslam_plane_t* planes, int first, int count);
static Bound make_bound(const float* b6) {
    Bound b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = b6[2 * k];
        b.hi[k] = b6[2 * k + 1];
    }
    return b;
}

extern "C" int eslam_sdf_grad(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                              const float* pts, int64_t N, int flags, float* sdf, float* grad, eslam_stream_t stream) {
    if (N < 0) {
        eslam_set_error("eslam_sdf_grad: negative N (%lld)", (long long)N);
        return 1;
    }
    if (flags & ~ESLAM_SDF_GRAD_UNIT) {
        eslam_set_error("eslam_sdf_grad: unknown flags 0x%x", flags);
        return 1;
    }
    if (N == 0) return 0;
    if (!planes || !dec || !bound6_host || !pts || !grad) {
        eslam_set_error("eslam_sdf_grad: null argument");
        return 1;
    }
    if (!dec->w1 || !dec->b1 || !dec->w2 || !dec->b2 || !dec->w3 || !dec->b3) {
        eslam_set_error("eslam_sdf_grad: null SDF decoder parameter");
        return 1;
    }
    if (eslam_validate_planes(planes, 0, 6)) return 1;
    GeoPlaneSet ps;
    for (int i = 0; i < 6; ++i) ps.p[i] = planes[i];
    const Bound bnd = make_bound(bound6_host);
    const bool cl = eslam_planes_channels_last(planes, 0, 6);
    const int64_t ntiles = (N + 63) / 64;
    const int64_t nwg = (ntiles + 3) / 4;
    dim3 grid((unsigned)(nwg < ESLAM_SDF_GRAD_MAX_GROUPS ? nwg : ESLAM_SDF_GRAD_MAX_GROUPS)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int unit = (flags & ESLAM_SDF_GRAD_UNIT) ? 1 : 0;
    eslam_prof_begin(PROF_SDF_GRAD, st);
    if (cl) hipLaunchKernelGGL((sdf_grad_kernel<true>), grid, block, 0, st, ps, *dec, bnd, pts, N, unit, sdf, grad);
    else hipLaunchKernelGGL((sdf_grad_kernel<false>), grid, block, 0, st, ps, *dec, bnd, pts, N, unit, sdf, grad);
    eslam_prof_end(PROF_SDF_GRAD, st);
    return eslam_check_launch("sdf_grad_kernel");
}
