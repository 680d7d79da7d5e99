// Backward kernels (K8 of SURVEY.md section 2.1): autograd of composite -> decoders -> tri-plane lookup.
//
//   decode_act_bwd_kernel  free points: g_raw -> pre-activation output grads g_o[N,4]
//   mlp_bwd_kernel         per ray (or 64-point tile of free points) and decoder: composite backward of the ray - upstream
//                          (g_depth, g_rgb, g_sdf), or the mapping loss's own gradient -> pre-activation output grads and
//                          g_beta, in registers - then the hidden layers, back-propagation to the 64 features (g_feat[N,128],
//                          or the rank-16 g_z1) and to the decoder parameters (per-workgroup slabs); fp32 or bf16 MFMA.
//                          Its phases: eslam_mlp_bwd_dev.h
//   beta_sum_kernel        g_beta's partials -> g_beta, when no slab reduction runs
//   dec_grad_reduce_kernel slabs -> flat decoder gradient
//   scatter (eslam_scatter.hip)  g_feat -> plane gradients
//   coord_bwd_kernel       optional: gradient w.r.t. the sample position -> rays_o / rays_d (pose) or points
//   coord_bwd_lowp_kernel  the same for the rays and the free points of the mixed-precision path, on the planes' half copies
#include <stdlib.h>
#include "eslam_decode_tile.h"
#include "eslam_loss_final.h"
#include "eslam_dec_reduce.h"
#include "eslam_mlp_bwd_dev.h"

// decode-mode variant: g_o = g_raw * activation'(raw)      (autograd of decoders.py:103,123)
__global__ void decode_act_bwd_kernel(const float* __restrict__ raw, const float* __restrict__ g_raw, int64_t N,
                                      float* __restrict__ g_o) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float4_t v = *(const float4_t*)(raw + 4 * i);
    const float4_t g = *(const float4_t*)(g_raw + 4 * i);
    float4_t o;
    o[0] = g[0] * v[0] * (1.0f - v[0]);
    o[1] = g[1] * v[1] * (1.0f - v[1]);
    o[2] = g[2] * v[2] * (1.0f - v[2]);
    o[3] = g[3] * (1.0f - v[3] * v[3]);
    *(float4_t*)(g_o + 4 * i) = o;
}

// ---------------------------------------------------------------------------------------------------------
// decoder MLP backward (eslam_mlp_bwd_dev.h)
// ---------------------------------------------------------------------------------------------------------
// MODE 0: tiles of 64 free points, pre-activation output gradients g_o [N,4] from memory (decode_act_bwd_kernel).
// MODE 1: a wave owns a RAY: it runs the composite backward of its chunks (upstream gradients from memory) and feeds the
//         result to the MLP backward from registers - the sample role of the one IS the B operand of the other.  Both
//         decoders' workgroups (blockIdx.y) repeat the scalar composite work; neither writes g_o.
// MODE 2: as 1, and the upstream gradients are those of the mapping loss (src/Mapper.py:110-144,337-346), formed here from
//         the global set sizes in li.acc: loss gradient, composite backward and decoder backward are ONE launch.
// WGRAD = false: decoders are frozen (tracking, reference src/Tracker.py:111-112): only g_feat is produced, the
// parameter-gradient contractions (28 of the 68 MFMAs per block), their LDS transposes and the slabs are skipped.
// LOWP: the mixed-precision tile (eslam_decode_tile.h): hidden layers recomputed and every product of the backward pass on
// bf16 MFMA (16x16x32 / 16x16x16) with float32 accumulation - 15 MFMAs of 16 cycles per 16 points and decoder instead of
// 68 of 32 cycles; features, activations' masks, biases and all accumulators stay float32.
// MODE 0 with LOWP (free points, eslam_decode_bwd on half copies; saved features bf16): WGRAD 159 VGPRs and 66.6 KB of LDS -
// two workgroups per CU, i.e. the 2 waves per SIMD of the bound, are what the LDS allows; frozen decoders 90 VGPRs, 15 KB,
// 5 waves per SIMD (the bound is a floor).  Neither uses scratch.
// GZ (float32 rays whose positions need no gradient, plane gradients wanted, not deterministic): the features' gradient is
// g_feat = W1^T . g_z1 and has rank 16, and the scatter is linear - so the product is NOT formed here (16 of a block's 76
// dependent MFMAs, 12 of its 16 ds_bpermute, three of its four 16-byte stores per lane: what is left is the move of g_z1's four
// registers to the gather role and one store).  The block's g_z1 is stored, gz[2][N][16]
// (decoder-major: a 128-byte line holds two consecutive samples of one ray), in the region g_feat occupies otherwise and a
// quarter of its size; scatter_sort_kernel<GZ> sums it per texel cell and expands each cell's sums once.
// SAVEDH (float32 rays, the forward pass saved its first hidden layer: `hid`, layout at hidden_blocks in eslam_decode_tile.h):
// h1 is READ - one 16-byte load per lane and block, requested a block ahead with the block's feature rows - instead of being
// rebuilt from the features: 16 of a block's 52 dependent MFMAs (GZ), the 16 ds_bpermute that moved the features to the MFMA
// role and the 16 registers of the W1 fragment go; h2 is still recomputed from h1 (4 MFMAs).  Same instructions on the same
// values as in the forward pass, so every output keeps its bits.  The features are still read for the g_W1 contraction (through
// the wave-private LDS tile, gather role); with frozen decoders (WGRAD = false) they are not read at all.
template <int MODE, bool WGRAD, bool LOWP, bool GZ = false, bool SAVEDH = false>
__global__ __launch_bounds__(256, 2) void mlp_bwd_kernel(const MlpBwdArgs a) {
    static_assert(!GZ || (!LOWP && MODE != 0), "GZ: float32 rays only");
    static_assert(!SAVEDH || (!LOWP && MODE != 0), "SAVEDH: float32 rays only");
    constexpr bool ROWS = !SAVEDH || WGRAD;           // the block's feature rows are read
    __shared__ MlpBwdLds<MODE, WGRAD, LOWP> lds;
    if (LOWP) stage_decoder_weights_lowp(lds.wlds, a.dec, threadIdx.x, blockDim.x);
    else stage_decoder_weights(lds.wlds, a.dec, threadIdx.x, blockDim.x);
    __syncthreads();

    const MlpBwdLane ln = mlp_bwd_lane();
    MlpBwdFrag<LOWP, GZ> w;
    w.load(lds.wlds, ln);
    MlpBwdParamGrads pg;
    pg.clear();
    const MlpBwdGradOut<GZ> out(a.g_feat, a.N, ln);
    MlpBwdPrefetch<LOWP, ROWS, SAVEDH> pf;

    if constexpr (MODE == 0) {
        mlp_bwd_points<WGRAD, LOWP>(a, lds, ln, w, pg, out, pf);
    } else {
        const float gbeta_acc = mlp_bwd_rays<MODE, WGRAD, LOWP, GZ, SAVEDH>(a, lds, ln, w, pg, out, pf);
        mlp_bwd_beta_partial(lds.beta_part, a.rb.beta_parts, gbeta_acc, ln);
    }
    if constexpr (WGRAD) pg.write_slab(lds.comb, a.slabs, ln);
}

__global__ __launch_bounds__(1024) void beta_sum_kernel(const float* __restrict__ parts, int n, float* __restrict__ out) {
    __shared__ float bsum[16];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) a += parts[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) bsum[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += bsum[k];
        out[0] = t;
    }
}

// slabs [nrows][2][SLAB] -> g_dec: eslam_dec_reduce.h.  Stand-alone launch, used when the scatter cannot carry the work
// (no plane gradients requested, deterministic mode, free points).
__global__ __launch_bounds__(1024) void dec_grad_reduce_kernel(const DecReduceArgs a) {
    __shared__ float red[16 * 64];
    dec_grad_reduce_block<1024>(a, blockIdx.x, blockIdx.y, red);
}

// ---------------------------------------------------------------------------------------------------------
// gradient w.r.t. sample positions (autograd of the grid coordinates + common.py:215-217 + Renderer.py:136-137)
// ---------------------------------------------------------------------------------------------------------
template <bool CL>
__device__ __forceinline__ void coord_grad8(const eslam_plane_t& P, float u, float v, int q, const float g[8],
                                            float& gu, float& gv) {
    // q: the lane's piece of the texel (gather role): channels piece_channel(q, 0..7)
    const AxisCoord ax = axis_coord(u, P.w);
    const AxisCoord ay = axis_coord(v, P.h);
    const int sy = (int)P.stride_y, sx = (int)P.stride_x, sc = (int)P.stride_c;
    const int r0 = ay.i0 * sy, r1 = ay.i1 * sy, c0 = ax.i0 * sx, c1 = ax.i1 * sx;
    float su = 0.f, sv = 0.f;
    if (CL) {
        const float* base = P.data + 4 * q;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const float4_t t00 = *(const float4_t*)(base + r0 + c0 + 16 * hh);
            const float4_t t01 = *(const float4_t*)(base + r0 + c1 + 16 * hh);
            const float4_t t10 = *(const float4_t*)(base + r1 + c0 + 16 * hh);
            const float4_t t11 = *(const float4_t*)(base + r1 + c1 + 16 * hh);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                su += g[4 * hh + i] * ((t01[i] - t00[i]) * (1.0f - ay.t) + (t11[i] - t10[i]) * ay.t);
                sv += g[4 * hh + i] * ((t10[i] - t00[i]) * (1.0f - ax.t) + (t11[i] - t01[i]) * ax.t);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* b = P.data + piece_channel(q, i) * sc;
            const float t00 = b[r0 + c0], t01 = b[r0 + c1], t10 = b[r1 + c0], t11 = b[r1 + c1];
            su += g[i] * ((t01 - t00) * (1.0f - ay.t) + (t11 - t10) * ay.t);
            sv += g[i] * ((t10 - t00) * (1.0f - ax.t) + (t11 - t01) * ax.t);
        }
    }
    // d(ix)/du = (w-1)/2 strictly inside, 0 where the border clamp is active (ATen clip_coordinates_set_grad)
    gu += ax.inside ? su * (0.5f * (float)(P.w - 1)) : 0.0f;
    gv += ay.inside ? sv * (0.5f * (float)(P.h - 1)) : 0.0f;
}

template <bool CL, bool RENDER>
__global__ __launch_bounds__(256, 2) void coord_bwd_kernel(const PlaneSet planes, const Bound bnd,
                                                        const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d,
                                                        const float* __restrict__ z_vals, int R, int S,
                                                        const float* __restrict__ g_feat,
                                                        float* __restrict__ g_rays_o, float* __restrict__ g_rays_d) {
    // RENDER: one wave per ray, outputs g_rays_o/g_rays_d [R,3].
    // else:   one wave per 64 points (z_vals = pts [N,3], R = N), output g_rays_o = g_pts [N,3].
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = gather_point<CL>(lane), q = gather_piece<CL>(lane);     // gather role (eslam_decode_tile.h)
    const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
    const int64_t nunits = RENDER ? R : ((int64_t)R + 63) / 64;
    if (unit >= nunits) return;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (RENDER) {
        ox = rays_o[unit * 3 + 0]; oy = rays_o[unit * 3 + 1]; oz = rays_o[unit * 3 + 2];
        dx = rays_d[unit * 3 + 0]; dy = rays_d[unit * 3 + 1]; dz = rays_d[unit * 3 + 2];
    }
    const int64_t base = RENDER ? unit * S : unit * 64;
    const int scount = RENDER ? S : (int)min((int64_t)64, (int64_t)R - base);
    const float sc3[3] = {2.0f / (bnd.hi[0] - bnd.lo[0]), 2.0f / (bnd.hi[1] - bnd.lo[1]), 2.0f / (bnd.hi[2] - bnd.lo[2])};
    float go_acc[3] = {0.f, 0.f, 0.f}, gd_acc[3] = {0.f, 0.f, 0.f};
    bool live = false;                        // some sample of the ray carries a position gradient that is not exactly zero
#pragma unroll 1
    for (int s0 = 0; s0 < scount; s0 += 16) {
        const int oz0 = opaque_zero(s0);      // keeps the 12 planes' scalar loads inside this loop (see gather_features)
        const int s = s0 + r;
        const bool valid = s < scount;
        const int sc_ = min(s, scount - 1);
        float x, y, z, zz = 0.f;
        if (RENDER) {
            zz = z_vals[base + sc_];
            x = ox + dx * zz; y = oy + dy * zz; z = oz + dz * zz;
        } else {
            x = z_vals[(base + sc_) * 3 + 0]; y = z_vals[(base + sc_) * 3 + 1]; z = z_vals[(base + sc_) * 3 + 2];
        }
        x = norm_coord(x, bnd.lo[0], bnd.hi[0]);
        y = norm_coord(y, bnd.lo[1], bnd.hi[1]);
        z = norm_coord(z, bnd.lo[2], bnd.hi[2]);
        float gp[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
#pragma unroll
            for (int lvl = 0; lvl < 2; ++lvl) {
                const float* gfp = g_feat + (base + sc_) * 128 + d * 64 + lvl * 32 + 4 * q;
                const float4_t ga = *(const float4_t*)gfp, gb = *(const float4_t*)(gfp + 16);
                const float g[8] = {ga[0], ga[1], ga[2], ga[3], gb[0], gb[1], gb[2], gb[3]};
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    const eslam_plane_t& P = planes.p[2 * (3 * d + o) + lvl + oz0];
                    float gu = 0.f, gv = 0.f;
                    coord_grad8<CL>(P, ORIENT_U(o, x, y, z), ORIENT_V(o, x, y, z), q, g, gu, gv);
                    __builtin_amdgcn_sched_barrier(0);
                    gp[o == 2 ? 1 : 0] += gu;      // first coordinate: x (xy, xz) or y (yz)
                    gp[o == 0 ? 1 : 2] += gv;      // second coordinate: y (xy) or z (xz, yz)
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = gp[k];
            v += __shfl_xor(v, CL ? 1 : 16, WAVE);  // sum the four pieces of the point
            v += __shfl_xor(v, CL ? 2 : 32, WAVE);
            v = valid ? v * sc3[k] : 0.0f;
            if (RENDER) {
                if (q == 0) { go_acc[k] += v; gd_acc[k] += v * zz; }
                live = live || !(v == 0.0f);
            } else if (q == 0 && valid) {
                g_rays_o[(base + s) * 3 + k] = v;
            }
        }
    }
    if (RENDER) {
        const bool any_live = __ballot(live) != 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = wave_sum(go_acc[k]);
            const float b = wave_sum(gd_acc[k]);
            if (lane == 0) {
                g_rays_o[unit * 3 + k] = a;
                // a ray none of whose samples carries gradient (masked out by the loss) gets a hard zero, not the sum of 0 * z:
                // its z_vals may be anything - the NaN row of a ray whose AABB exit is 0/0
                g_rays_d[unit * 3 + k] = any_live ? b : 0.0f;
            }
        }
    }
}

// Mixed precision: the same gradient on the planes' half copies.  What the forward pass interpolated ARE the fp16-rounded
// texels (gather8_half), so the derivative of the bilinear form acts on them, not on the float32 masters; the roundings of
// planes and features pass gradients through.  Gather role of the mixed-precision tile: piece g = channels 8g..8g+7 of a
// level, one 16-byte load per corner (a quad of lanes one 64-byte texel).  Arithmetic, gates and factors are coord_grad8's.
__device__ __forceinline__ void coord_grad8_half(const eslam_plane_t& P, float u, float v, int g, const float gf[8],
                                                 float& gu, float& gv) {
    const AxisCoord ax = axis_coord(u, P.w);
    const AxisCoord ay = axis_coord(v, P.h);
    const unsigned sy = (unsigned)P.stride_y, sx = (unsigned)P.stride_x;
    const unsigned r0 = ay.i0 * sy, r1 = ay.i1 * sy, c0 = ax.i0 * sx, c1 = ax.i1 * sx, g8 = 8u * g;
    const _Float16* __restrict__ data = (const _Float16*)P.data_f16;
    const half8_t t00 = *(const half8_t*)(data + r0 + c0 + g8);
    const half8_t t01 = *(const half8_t*)(data + r0 + c1 + g8);
    const half8_t t10 = *(const half8_t*)(data + r1 + c0 + g8);
    const half8_t t11 = *(const half8_t*)(data + r1 + c1 + g8);
    float su = 0.f, sv = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float a00 = (float)t00[i], a01 = (float)t01[i], a10 = (float)t10[i], a11 = (float)t11[i];
        su += gf[i] * ((a01 - a00) * (1.0f - ay.t) + (a11 - a10) * ay.t);
        sv += gf[i] * ((a10 - a00) * (1.0f - ax.t) + (a11 - a01) * ax.t);
    }
    gu += ax.inside ? su * (0.5f * (float)(P.w - 1)) : 0.0f;
    gv += ay.inside ? sv * (0.5f * (float)(P.h - 1)) : 0.0f;
}

// RENDER: one wave per ray (the RENDER mode of coord_bwd_kernel), 48 texel loads per sample where the float32 kernel issues 96.
// else:   one wave per 64 free points in four passes of 16, four lanes per point (z_vals = pts [N,3], R = N); g_rays_o =
//         g_pts [N,3], written directly.
// g_feat stays float32 in natural channel order (written by the LOWP mlp_bwd_kernel for the scatter): the lane's 8
// channels of a level are two adjacent 16-byte loads.  No LDS.  RENDER: 166 VGPRs, 3 waves per SIMD (as the float32 kernel,
// 152): asked for 4 waves (128 VGPRs) the compiler spills 27 registers to scratch inside the sample loop, so 3 is what is asked.
// Points: 152 VGPRs, no scratch, 3 waves per SIMD under the same bound.
template <bool RENDER>
__global__ __launch_bounds__(256, 3) void coord_bwd_lowp_kernel(const PlaneSet planes, const Bound bnd,
                                                                const float* __restrict__ rays_o,
                                                                const float* __restrict__ rays_d,
                                                                const float* __restrict__ z_vals, int R, int S,
                                                                const float* __restrict__ g_feat,
                                                                float* __restrict__ g_rays_o, float* __restrict__ g_rays_d) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane >> 2, g = lane & 3;                 // gather role of the mixed-precision tile
    // points: the wave's index is wave-uniform; say so, so that the trip count and the rows (functions of it, not of S) are
    // scalar and the loop's branch is a scalar one
    const int64_t unit = (int64_t)blockIdx.x * 4 + (RENDER ? wave : __builtin_amdgcn_readfirstlane(wave));
    const int64_t nunits = RENDER ? R : ((int64_t)R + 63) / 64;
    if (unit >= nunits) return;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f;
    if (RENDER) {
        ox = rays_o[unit * 3 + 0]; oy = rays_o[unit * 3 + 1]; oz = rays_o[unit * 3 + 2];
        dx = rays_d[unit * 3 + 0]; dy = rays_d[unit * 3 + 1]; dz = rays_d[unit * 3 + 2];
    }
    const int64_t base = RENDER ? unit * S : unit * 64;
    const int scount = RENDER ? S : (int)min((int64_t)64, (int64_t)R - base);
    const float sc3[3] = {2.0f / (bnd.hi[0] - bnd.lo[0]), 2.0f / (bnd.hi[1] - bnd.lo[1]), 2.0f / (bnd.hi[2] - bnd.lo[2])};
    float go_acc[3] = {0.f, 0.f, 0.f}, gd_acc[3] = {0.f, 0.f, 0.f};
    bool live = false;                        // some sample of the ray carries a position gradient that is not exactly zero
#pragma unroll 1
    for (int s0 = 0; s0 < scount; s0 += 16) {
        const int oz0 = opaque_zero(s0);      // keeps the 12 planes' scalar loads inside this loop (see gather_features)
        const int s = s0 + r;
        const bool valid = s < scount;
        const int sc_ = min(s, scount - 1);
        float x, y, z, zz = 0.f;
        if (RENDER) {
            zz = z_vals[base + sc_];
            x = ox + dx * zz; y = oy + dy * zz; z = oz + dz * zz;
        } else {
            x = z_vals[(base + sc_) * 3 + 0]; y = z_vals[(base + sc_) * 3 + 1]; z = z_vals[(base + sc_) * 3 + 2];
        }
        x = norm_coord(x, bnd.lo[0], bnd.hi[0]);
        y = norm_coord(y, bnd.lo[1], bnd.hi[1]);
        z = norm_coord(z, bnd.lo[2], bnd.hi[2]);
        float gp[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 2; ++d) {
#pragma unroll
            for (int lvl = 0; lvl < 2; ++lvl) {
                const float* gfp = g_feat + (base + sc_) * 128 + d * 64 + lvl * 32 + 8 * g;
                const float4_t ga = *(const float4_t*)gfp, gb = *(const float4_t*)(gfp + 4);
                const float gf[8] = {ga[0], ga[1], ga[2], ga[3], gb[0], gb[1], gb[2], gb[3]};
#pragma unroll
                for (int o = 0; o < 3; ++o) {
                    const eslam_plane_t& P = planes.p[2 * (3 * d + o) + lvl + oz0];
                    float gu = 0.f, gv = 0.f;
                    coord_grad8_half(P, ORIENT_U(o, x, y, z), ORIENT_V(o, x, y, z), g, gf, gu, gv);
                    __builtin_amdgcn_sched_barrier(0);
                    gp[o == 2 ? 1 : 0] += gu;      // first coordinate: x (xy, xz) or y (yz)
                    gp[o == 0 ? 1 : 2] += gv;      // second coordinate: y (xy) or z (xz, yz)
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = gp[k];
            v += __shfl_xor(v, 1, WAVE);            // sum the four pieces of the point
            v += __shfl_xor(v, 2, WAVE);
            v = valid ? v * sc3[k] : 0.0f;
            if (RENDER) {
                if (g == 0) { go_acc[k] += v; gd_acc[k] += v * zz; }
                live = live || !(v == 0.0f);
            } else if (g == (s0 >> 4)) {
                // all four lanes of a point hold its sum: lane (r, g) keeps that of pass g, i.e. of point 16 g + r, and the wave
                // writes its 64 points once behind the loop.  (With the stores inside the loop, as in the float32 kernel's point
                // mode, the compiler spilled ~280 registers around them: 1.1 KB of scratch per lane at either bound.)
                go_acc[k] = v;
            }
        }
    }
    if (RENDER) {
        const bool any_live = __ballot(live) != 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = wave_sum(go_acc[k]);
            const float b = wave_sum(gd_acc[k]);
            if (lane == 0) {
                g_rays_o[unit * 3 + k] = a;
                // a ray none of whose samples carries gradient (masked out by the loss) gets a hard zero, not the sum of 0 * z:
                // its z_vals may be anything - the NaN row of a ray whose AABB exit is 0/0
                g_rays_d[unit * 3 + k] = any_live ? b : 0.0f;
            }
        }
    } else if (16 * g + r < scount) {
        float* dst = g_rays_o + (base + 16 * g + r) * 3;
        dst[0] = go_acc[0]; dst[1] = go_acc[1]; dst[2] = go_acc[2];
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
bool eslam_planes_channels_last(const eslam_plane_t* planes, int first, int count);
int eslam_validate_planes(const eslam_plane_t* planes, int first, int count);
int eslam_planes_lowp(const eslam_plane_t* planes);

static Bound make_bound(const float* b6) {
    Bound b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = b6[2 * k];
        b.hi[k] = b6[2 * k + 1];
    }
    return b;
}

#define MLP_BWD_MAX_WG 256

int eslam_scatter_v2(const eslam_plane_t* planes, const Bound& bnd, const float* rays_o, const float* rays_d,
                     const float* z_or_pts, int64_t R, int S, bool render, const float* g_feat, const int* perm,
                     hipStream_t st, const DecReduceArgs* red, const eslam_decoders_t* gz_dec);
bool eslam_scatter_can_reduce(bool render);


static int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// workspace layout: g_o [n,4] | g_feat [n,128] (rank-16 path: g_z1 [2][n,16] in its first quarter) | slabs [MLP_BWD_MAX_WG*4][2][SLAB] + g_beta partials [n/4 + 1] |
//                   ray order [n] (int)
struct BwdWorkspace {
    float* g_o;
    float* g_feat;
    float* slabs;                  // the g_beta partials follow the slabs: bwd_beta_parts
    int* order;
};
static int64_t slab_region_bytes(int64_t n_points) {
    return ((int64_t)MLP_BWD_MAX_WG * 4 * 2 * SLAB + n_points / 4 + 1) * 4;      // (g_beta partials need MLP_BWD_MAX_WG only)
}
static float* bwd_beta_parts(float* slabs) { return slabs + (int64_t)MLP_BWD_MAX_WG * 4 * 2 * SLAB; }
// the four regions of a workspace for n_points (regions: may be NULL); returns the bytes they take
static int64_t bwd_workspace(int64_t n_points, void* workspace, BwdWorkspace* regions) {
    const int64_t o_feat = align256(n_points * 4 * 4), o_slabs = o_feat + align256(n_points * 128 * 4);
    const int64_t o_order = o_slabs + align256(slab_region_bytes(n_points)), end = o_order + align256(n_points * 4);
    if (regions) {
        char* ws = (char*)workspace;
        regions->g_o = (float*)ws;
        regions->g_feat = (float*)(ws + o_feat);
        regions->slabs = (float*)(ws + o_slabs);
        regions->order = (int*)(ws + o_order);
    }
    return end;
}

extern "C" int64_t eslam_bwd_workspace_bytes(int64_t n_points) {
    if (n_points < 0) return -1;
    return bwd_workspace(n_points, nullptr, nullptr);
}

// 1 when the last backward this process dispatched took the rank-16 pair, 0 when it wrote full-width rows (host bookkeeping)
static int g_last_backward_rank16 = 0;
extern "C" int eslam_last_backward_rank16(void) { return g_last_backward_rank16; }
// 1 when it read the forward pass's saved first hidden layer, 0 when it recomputed it
static int g_last_backward_saved_hidden = 0;
extern "C" int eslam_last_backward_saved_hidden(void) { return g_last_backward_saved_hidden; }

// The 24 instantiations of mlp_bwd_kernel the host reaches: mixed precision (no GZ, no SAVEDH) x 3 modes, float32 free points, and
// float32 rays x 2 modes x GZ x SAVEDH - each with trainable and with frozen decoders.
template <int MODE, bool LOWP, bool GZ, bool SAVEDH>
static void mlp_bwd_launch(bool wgrad, int nwg, hipStream_t st, const MlpBwdArgs& a) {
    if (wgrad) hipLaunchKernelGGL((mlp_bwd_kernel<MODE, true, LOWP, GZ, SAVEDH>), dim3(nwg, 2), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((mlp_bwd_kernel<MODE, false, LOWP, GZ, SAVEDH>), dim3(nwg, 2), dim3(256), 0, st, a);
}
template <bool LOWP, bool GZ, bool SAVEDH>
static void mlp_bwd_launch_rays(int mode, bool wgrad, int nwg, hipStream_t st, const MlpBwdArgs& a) {
    if (mode == 1) mlp_bwd_launch<1, LOWP, GZ, SAVEDH>(wgrad, nwg, st, a);
    else mlp_bwd_launch<2, LOWP, GZ, SAVEDH>(wgrad, nwg, st, a);
}
static void mlp_bwd_dispatch(int mode, bool wgrad, bool lowp, bool gz, bool savedh, int nwg, hipStream_t st, const MlpBwdArgs& a) {
    if (lowp && mode == 0) mlp_bwd_launch<0, true, false, false>(wgrad, nwg, st, a);      // feat: [N,128] bf16
    else if (lowp) mlp_bwd_launch_rays<true, false, false>(mode, wgrad, nwg, st, a);
    else if (mode == 0) mlp_bwd_launch<0, false, false, false>(wgrad, nwg, st, a);
    else if (gz && savedh) mlp_bwd_launch_rays<false, true, true>(mode, wgrad, nwg, st, a);
    else if (gz) mlp_bwd_launch_rays<false, true, false>(mode, wgrad, nwg, st, a);
    else if (savedh) mlp_bwd_launch_rays<false, false, true>(mode, wgrad, nwg, st, a);
    else mlp_bwd_launch_rays<false, false, false>(mode, wgrad, nwg, st, a);
}

// One backward: what eslam_render_bwd* and eslam_decode_bwd hand to bwd_common
struct BwdPlan {
    int mode;                      // 0: free points (g_o in the workspace); 1: rays, upstream gradients in rb; 2: rays, mapping-loss gradients from li
    const eslam_plane_t* planes;
    const eslam_decoders_t* dec;
    Bound bnd;
    const float* rays_o;           // rays
    const float* rays_d;           // rays
    const float* z_or_pts;         // rays: z_vals [R,S]; free points: the points [R,3]
    int64_t R;                     // rays, or free points
    int S;                         // samples per ray
    const float* feat;             // the forward pass's features
    const float* hid;              // rays: its saved first hidden layer, or NULL
    BwdWorkspace ws;
    const int* perm;               // rays: the ray orders for the scatter, or NULL
    RayBwdIn rb;                   // rays
    const LossGradIn* li;          // mode 2
    float* g_dec;                  // out, or NULL: decoders are frozen
    float* g_beta;                 // out, or NULL
    float* g_out_a;                // out, or NULL: g_rays_o [R,3], free points: g_pts [R,3]
    float* g_out_b;                // out, or NULL: g_rays_d [R,3]
    hipStream_t st;
};

static int bwd_common(const BwdPlan& p) {
    const eslam_plane_t* planes = p.planes;
    hipStream_t st = p.st;
    const bool render = p.mode != 0;
    const int64_t R = p.R;
    const int S = p.S;
    const int64_t N = render ? R * S : R;
    PlaneSet ps;
    for (int i = 0; i < NPL; ++i) ps.p[i] = planes[i];
    const bool cl = eslam_planes_channels_last(planes, 0, NPL);

    // decoder MLP backward (rays: with the composite backward, and the loss gradient, in the same launch)
    const int64_t ntiles = render ? R : (N + 63) / 64;                 // a wave's unit of work: a ray, or 64 free points
    const int nwg = (int)((ntiles + 3) / 4 < MLP_BWD_MAX_WG ? (ntiles + 3) / 4 : MLP_BWD_MAX_WG);
    float* beta_parts = bwd_beta_parts(p.ws.slabs);
    if (N * 512 >= ((int64_t)1 << 32) - 256) {     // the feature-gradient rows are addressed with 32-bit byte offsets (as in the scatter)
        eslam_set_error("backward: %lld points exceed the 32-bit offset range of the feature-gradient buffer (8.3 M): split the batch",
                        (long long)N);
        return 1;
    }
    eslam_prof_begin(PROF_MLP_BWD, st);
    const int lowp = eslam_planes_lowp(planes);
    if (lowp < 0) return 1;
    bool any_grad = false, all_grad = true;
    for (int i = 0; i < NPL; ++i) {
        any_grad |= planes[i].grad != nullptr;
        all_grad &= planes[i].grad != nullptr;
    }
    if (any_grad && !all_grad) {
        eslam_set_error("plane gradients must be requested for all 12 planes or for none");
        return 1;
    }
    // The rank-16 pair (mlp_bwd_kernel<GZ> writes g_z1, scatter_sort_kernel<GZ> expands per cell): float32 rays whose
    // feature gradients only the scatter reads.  Position gradients (coord_bwd_kernel reads full rows), free points, the
    // mixed-precision kernels and deterministic mode (fixed point per CONTRIBUTION) keep the full-width rows.
    const bool gz = !lowp && render && any_grad && !p.g_out_a && !eslam_deterministic();
    g_last_backward_rank16 = gz ? 1 : 0;
    const float* hid = (lowp || !render) ? nullptr : p.hid;        // (mixed precision and free points save no hidden layer)
    g_last_backward_saved_hidden = hid ? 1 : 0;
    MlpBwdArgs a = {};
    a.dec = *p.dec; a.feat = p.feat; a.g_o = p.ws.g_o; a.N = N; a.g_feat = p.ws.g_feat; a.slabs = p.ws.slabs;
    a.rb = p.rb; a.rb.beta_parts = render ? beta_parts : nullptr;
    if (p.li) a.li = *p.li;
    a.hid = hid;
    mlp_bwd_dispatch(p.mode, p.g_dec != nullptr, lowp != 0, gz, hid != nullptr, nwg, st, a);
    eslam_prof_end(PROF_MLP_BWD, st);
    if (int rc = eslam_check_launch("mlp_bwd_kernel")) return rc;
    const int n_beta_parts = render ? nwg : 0;
    DecReduceArgs red = {};
    red.slabs = p.ws.slabs; red.nrows = nwg; red.g_dec = p.g_dec;
    red.beta_parts = render ? beta_parts : nullptr; red.n_beta_parts = n_beta_parts; red.g_beta = p.g_beta;
    // The slab reduction (44 workgroups, latency-bound, ~7 us as a launch of its own) rides in the scatter's grid when there
    // is one: its workgroups run beside the scatter's first ones instead of in front of them.
    const bool fold = p.g_dec && any_grad && eslam_scatter_can_reduce(render);
    if (p.g_dec && !fold) {
        eslam_prof_begin(PROF_DEC_REDUCE, st);
        hipLaunchKernelGGL(dec_grad_reduce_kernel, dim3(DEC_RED_COLBLOCKS, 2), dim3(1024), 0, st, red);
        eslam_prof_end(PROF_DEC_REDUCE, st);
        if (int rc = eslam_check_launch("dec_grad_reduce_kernel")) return rc;
    } else if (!p.g_dec && p.g_beta && render) {      // beta's gradient does not go through the decoders: still sum its partials
        hipLaunchKernelGGL(beta_sum_kernel, dim3(1), dim3(1024), 0, st, beta_parts, n_beta_parts, p.g_beta);
        if (int rc = eslam_check_launch("beta_sum_kernel")) return rc;
    }

    // plane gradients
    if (any_grad) {
        eslam_prof_begin(PROF_SCATTER, st);
        if (int rc = eslam_scatter_v2(planes, p.bnd, p.rays_o, p.rays_d, p.z_or_pts, R, S, render, p.ws.g_feat, p.perm, st,
                                      fold ? &red : nullptr, gz ? p.dec : nullptr))
            return rc;
        eslam_prof_end(PROF_SCATTER, st);
    }
    // position gradients
    if (p.g_out_a) {
        const int64_t nunits = render ? R : (N + 63) / 64;
        dim3 grid((unsigned)((nunits + 3) / 4)), block(256);
#define LAUNCH(...)                                                                                                     \
    hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, st, ps, p.bnd, p.rays_o, p.rays_d, p.z_or_pts, (int)R, S, p.ws.g_feat, \
                       p.g_out_a, p.g_out_b)
        eslam_prof_begin(PROF_COORD_BWD, st);
        if (lowp && render) LAUNCH(coord_bwd_lowp_kernel<true>);      // (channels-last half copies: checked by eslam_planes_lowp)
        else if (lowp) LAUNCH(coord_bwd_lowp_kernel<false>);
        else if (cl && render) LAUNCH(coord_bwd_kernel<true, true>);
        else if (cl) LAUNCH(coord_bwd_kernel<true, false>);
        else if (render) LAUNCH(coord_bwd_kernel<false, true>);
        else LAUNCH(coord_bwd_kernel<false, false>);
#undef LAUNCH
        eslam_prof_end(PROF_COORD_BWD, st);
        if (int rc = eslam_check_launch("coord_bwd_kernel")) return rc;
    }
    return 0;
}

static int render_bwd_impl(const char* who, const eslam_plane_t* planes, const eslam_decoders_t* dec,
                           const float* bound6_host, const float* rays_o, const float* rays_d, const float* z_vals, int R,
                           int S, const float* sdf, const float* raw_rgb, const float* feat, const float* g_depth,
                           const float* g_rgb, const float* g_sdf, const LossGradIn* li, float* g_dec, float* g_beta,
                           float* g_rays_o, float* g_rays_d, const int32_t* ray_order, void* workspace, const float* hid,
                           eslam_stream_t stream) {
    if (R <= 0) return 0;
    if (S <= 0 || S > ESLAM_MAX_SAMPLES) {
        eslam_set_error("%s: S=%d outside [1,%d]", who, S, ESLAM_MAX_SAMPLES);
        return 1;
    }
    if (!planes || !dec || !bound6_host || !rays_o || !rays_d || !z_vals || !sdf || !raw_rgb || !feat || !workspace) {
        eslam_set_error("%s: null argument", who);
        return 1;
    }
    if ((g_rays_o == nullptr) != (g_rays_d == nullptr)) {
        eslam_set_error("%s: g_rays_o and g_rays_d must both be given or both be NULL", who);
        return 1;
    }
    if ((int64_t)R * S * 128 >= ((int64_t)1 << 40)) {
        eslam_set_error("%s: batch too large", who);
        return 1;
    }
    if (eslam_validate_planes(planes, 0, NPL)) return 1;
    BwdPlan p = {};
    p.mode = li ? 2 : 1;
    p.planes = planes; p.dec = dec; p.bnd = make_bound(bound6_host);
    p.rays_o = rays_o; p.rays_d = rays_d; p.z_or_pts = z_vals; p.R = R; p.S = S;
    p.feat = feat; p.hid = hid;
    p.st = (hipStream_t)stream;
    const int64_t N = (int64_t)R * S;
    bwd_workspace(N, workspace, &p.ws);
    p.perm = ray_order;
    bool scatter_runs = false;         // the order bundles rays for the plane-gradient scatter: tracking (no plane gradients) has no use for it
    for (int i = 0; i < NPL; ++i) scatter_runs = scatter_runs || planes[i].grad != nullptr;
    if (!p.perm && scatter_runs && (int64_t)ESLAM_RAY_ORDER_WORDS(R) <= N) {      // the forward pass did not leave the orders: compute them here (in a region of R S ints)
        if (int rc = eslam_ray_order(rays_o, rays_d, R, p.ws.order, p.st)) return rc;
        p.perm = p.ws.order;
    }
    p.rb.z_vals = z_vals; p.rb.sdf = sdf; p.rb.raw_rgb = raw_rgb; p.rb.beta = dec->beta;
    p.rb.g_depth = g_depth; p.rb.g_rgb = g_rgb; p.rb.g_sdf = g_sdf; p.rb.R = R; p.rb.S = S;
    p.li = li;
    p.g_dec = g_dec; p.g_beta = g_beta; p.g_out_a = g_rays_o; p.g_out_b = g_rays_d;
    return bwd_common(p);
}

extern "C" int eslam_render_bwd_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                  const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                  const float* sdf, const float* raw_rgb, const float* feat, const float* g_depth,
                                  const float* g_rgb, const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o,
                                  float* g_rays_d, const int32_t* ray_order, void* workspace, const float* hidden,
                                  eslam_stream_t stream) {
    return render_bwd_impl("eslam_render_bwd", planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, sdf, raw_rgb, feat,
                           g_depth, g_rgb, g_sdf, nullptr, g_dec, g_beta, g_rays_o, g_rays_d, ray_order, workspace, hidden, stream);
}

extern "C" int eslam_render_bwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                const float* sdf, const float* raw_rgb, const float* feat, const float* g_depth,
                                const float* g_rgb, const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o,
                                float* g_rays_d, const int32_t* ray_order, void* workspace, eslam_stream_t stream) {
    return eslam_render_bwd_h(planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, sdf, raw_rgb, feat, g_depth, g_rgb, g_sdf,
                              g_dec, g_beta, g_rays_o, g_rays_d, ray_order, workspace, nullptr, stream);
}

extern "C" int eslam_render_bwd_loss_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                       const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                       const float* sdf, const float* raw_rgb, const float* feat, const float* depth,
                                       const float* rgb, const float* gt_depth, const float* gt_color, double truncation,
                                       const float* weights5_host, const uint8_t* ray_mask, const float* acc,
                                       const float* upstream, float* loss_out, const float* g_depth, const float* g_rgb,
                                       const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o, float* g_rays_d,
                                       const int32_t* ray_order, void* workspace, const float* hidden,
                                       eslam_stream_t stream) {
    if (!depth || !rgb || !gt_depth || !gt_color || !weights5_host || !acc) {
        eslam_set_error("eslam_render_bwd_loss: null loss argument");
        return 1;
    }
    LossGradIn li = {};
    li.gt_depth = gt_depth; li.gt_color = gt_color; li.ray_mask = ray_mask; li.depth = depth; li.rgb = rgb;
    li.acc = acc; li.upstream = upstream; li.loss_out = loss_out;
    li.tr = make_trunc(truncation);
    li.w = LossW{weights5_host[0], weights5_host[1], weights5_host[2], weights5_host[3], weights5_host[4]};
    return render_bwd_impl("eslam_render_bwd_loss", planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, sdf, raw_rgb,
                           feat, g_depth, g_rgb, g_sdf, &li, g_dec, g_beta, g_rays_o, g_rays_d, ray_order, workspace, hidden, stream);
}

extern "C" int eslam_render_bwd_loss(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                     const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                     const float* sdf, const float* raw_rgb, const float* feat, const float* depth,
                                     const float* rgb, const float* gt_depth, const float* gt_color, double truncation,
                                     const float* weights5_host, const uint8_t* ray_mask, const float* acc,
                                     const float* upstream, float* loss_out, const float* g_depth, const float* g_rgb,
                                     const float* g_sdf, float* g_dec, float* g_beta, float* g_rays_o, float* g_rays_d,
                                     const int32_t* ray_order, void* workspace, eslam_stream_t stream) {
    return eslam_render_bwd_loss_h(planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, sdf, raw_rgb, feat, depth, rgb, gt_depth,
                                   gt_color, truncation, weights5_host, ray_mask, acc, upstream, loss_out, g_depth, g_rgb, g_sdf,
                                   g_dec, g_beta, g_rays_o, g_rays_d, ray_order, workspace, nullptr, stream);
}

extern "C" int eslam_decode_bwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                const float* pts, int64_t N, const float* raw, const float* feat, const float* g_raw,
                                float* g_dec, float* g_pts, void* workspace, eslam_stream_t stream) {
    if (N <= 0) return 0;
    if (!planes || !dec || !bound6_host || !pts || !raw || !feat || !g_raw || !workspace) {
        eslam_set_error("eslam_decode_bwd: null argument");
        return 1;
    }
    if (N >= ((int64_t)1 << 31)) {
        eslam_set_error("eslam_decode_bwd: N too large");
        return 1;
    }
    if (eslam_validate_planes(planes, 0, NPL)) return 1;
    BwdPlan p = {};
    p.mode = 0;
    p.planes = planes; p.dec = dec; p.bnd = make_bound(bound6_host);
    p.z_or_pts = pts; p.R = N; p.S = 64;
    p.feat = feat;
    p.st = (hipStream_t)stream;
    bwd_workspace(N, workspace, &p.ws);
    p.g_dec = g_dec; p.g_out_a = g_pts;
    hipLaunchKernelGGL(decode_act_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, p.st, raw, g_raw, N, p.ws.g_o);
    if (int rc = eslam_check_launch("decode_act_bwd_kernel")) return rc;
    return bwd_common(p);
}
