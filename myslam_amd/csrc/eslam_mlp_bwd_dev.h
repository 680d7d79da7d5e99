// The phases of mlp_bwd_kernel (eslam_render_bwd.hip): decoder MLP backward (autograd of reference
// src/networks/decoders.py:97-103 / 117-123), with the composite backward (src/utils/Renderer.py:140-153) and - when the loss
// is the fused mapping loss - the loss gradient formed in the same wave.
//
//   MlpBwdArgs                    the kernel's one argument
//   MlpBwdLds                     the workgroup's LDS as one type
//   MlpBwdFragF32 / MlpBwdFragBf16  a decoder's weights on the lane, as the MFMAs of the backward pass want them
//   MlpBwdParamGrads              the wave's parameter-gradient accumulators and the epilogue that writes the slab row
//   MlpBwdGradOut                 the feature-gradient (GZ: g_z1) stores, always issued
//   MlpBwdPrefetch                a block's feature rows and saved h1, requested one block ahead
//   mlp_bwd_block_f32 / _bf16     one block of 16 points, out of its phases; mlp_bwd_tile loops over a tile's blocks
//   RayIn / ChunkIn / PassA, RayLossGrad, ray_pass_a, mlp_bwd_rays     MODE 1 and 2: a wave owns a ray
//   mlp_bwd_points                MODE 0: tiles of 64 free points
//
// Every piece is a type or a __forceinline__ function template; what a piece reads and changes is in its parameter list.
#pragma once
#include <type_traits>
#include "eslam_decode_tile.h"
#include "eslam_loss_final.h"

// ---------------------------------------------------------------------------------------------------------
// composite backward (autograd of reference src/utils/Renderer.py:140-153), one 64-sample chunk of one ray, sample role
// ---------------------------------------------------------------------------------------------------------
// Upstream of a ray: d L / d depth, d L / d rgb (gd, gr, gg, gb); per sample d L / d sdf (g_sdf_s).  Returns the
// pre-activation output gradients of the sample (o[0..2] colour, o[3] sdf) and adds to gbeta_acc.  `carry` is the suffix
// sum of gw*w over the LATER chunks (chunks are visited last to first), `trans_in` the transmittance entering the chunk.
struct RayUp { float gd, gr, gg, gb; };

__device__ __forceinline__ float4_t composite_bwd_chunk(const RayUp up, float beta, bool valid, float sd, float z, float cr,
                                                        float cg, float cb, float g_sdf_s, float trans_in, float& carry,
                                                        float& gbeta_acc, int lane) {
    const float sg = sigmoidf_(-sd * beta);
    const float e = expf(-beta * sg);
    const float alpha = valid ? 1.0f - e : 0.0f;
    const float fac = valid ? (1.0f - alpha) + 1e-10f : 1.0f;
    const float pin = wave_incl_prod(fac, lane);
    const float pex = wave_up1(pin, 1.0f);
    const float T = trans_in * pex;
    const float w = alpha * T;
    // a ray without a depth gradient (masked out, or depth-less under the mapping loss) contributes a hard zero, not 0 * z: its
    // z_vals may be anything - the NaN row of a ray whose AABB exit is 0/0 - and 0 * NaN would reach every gradient
    const float gw = (up.gd != 0.0f ? up.gd * z : 0.0f) + up.gr * cr + up.gg * cg + up.gb * cb;
    const float v = valid ? gw * w : 0.0f;
    // exclusive suffix sum_{k>i} gw_k w_k, formed WITHOUT subtracting v_i from an inclusive sum: w decays
    // geometrically along the ray, so (inclusive - own) would lose the small tail in the rounding of the
    // dominant own term, and g_alpha is itself a cancelling difference of two terms of the size of gw.
    const float vn = wave_down1(v, 0.0f);
    const float after_local = wave_incl_suffix_sum(vn, lane);
    const float after = after_local + carry;
    const float g_alpha = gw * T - after / fac;
    carry += wave_lane<0>(after_local) + wave_lane<0>(v);
    float4_t o = (float4_t){0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float ds = sg * (1.0f - sg);                // sigmoid'
        const float dalpha_dsdf = -beta * beta * e * ds;
        const float dalpha_dbeta = e * (sg - beta * ds * sd);
        gbeta_acc += g_alpha * dalpha_dbeta;
        const float g_sdf_tot = g_sdf_s + g_alpha * dalpha_dsdf;
        o[0] = w * up.gr * cr * (1.0f - cr);
        o[1] = w * up.gg * cg * (1.0f - cg);
        o[2] = w * up.gb * cb * (1.0f - cb);
        o[3] = g_sdf_tot * (1.0f - sd * sd);
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------
// arguments
// ---------------------------------------------------------------------------------------------------------
#define TP 20                      // row pitch (floats) of the 16x16 transpose tiles: conflict-free, 16-B aligned
#define TPF 68                     // row pitch of the 16-point x 64-feature tile (floats)
#define TPH 72                     // the same tile in bf16 (shorts): 144-byte rows keep the 16-byte writes aligned

struct RayBwdIn {                  // MODE >= 1: what the composite backward of a ray reads
    const float* z_vals;           // [R,S]
    const float* sdf;              // [R,S]   tanh outputs of the forward pass
    const float* raw_rgb;          // [R,S,3] sigmoid outputs
    const float* beta;             // [1]
    const float* g_depth;          // [R]   upstream, any of the three may be NULL (= 0); with MODE 2 they are ADDED to the
    const float* g_rgb;            // [R,3] loss's own gradients
    const float* g_sdf;            // [R,S]
    float* beta_parts;             // [gridDim.x] partial sums of g_beta (written by the sdf decoder's workgroups)
    int R, S;
};

// The kernel's one argument.  An instantiation reads only the fields of its mode (behind the `:`).  Every field is pointer- or
// int-sized: a wave-uniform BYTE of a by-value argument is fetched with a vector load and a v_readfirstlane.
struct MlpBwdArgs {
    eslam_decoders_t dec;
    const float* feat;             // the forward pass's features [N,128]: float32, LOWP: bf16
    const float* g_o;              // MODE 0: pre-activation output gradients [N,4] (decode_act_bwd_kernel)
    int64_t N;                     // points: R S, or the free points
    float* g_feat;                 // out: the features' gradient [N,128], GZ: g_z1 [2][N][16] in its first quarter
    float* slabs;                  // WGRAD: out, one row of partial parameter gradients per workgroup [gridDim.x][2][SLAB]
    RayBwdIn rb;                   // MODE 1, 2
    LossGradIn li;                 // MODE 2
    const float* hid;              // SAVEDH: the forward pass's first hidden layer (hidden_blocks in eslam_decode_tile.h)
};

// The lane's indices in the three roles a wave's lanes take
struct MlpBwdLane {
    int d;                         // blockIdx.y: 0 = sdf decoder, 1 = colour decoder
    int lane, wave;                // sample role: the lane is a point of the 64-point tile
    int r, q;                      // MFMA role
    int gp, gq;                    // gather role: feat / g_feat rows are read and written a quad per row (point gp, piece gq)
};

__device__ __forceinline__ MlpBwdLane mlp_bwd_lane() {
    MlpBwdLane ln;
    ln.d = blockIdx.y;
    ln.lane = threadIdx.x & 63; ln.wave = threadIdx.x >> 6;
    ln.r = ln.lane & 15; ln.q = ln.lane >> 4;
    ln.gp = ln.lane >> 2; ln.gq = ln.lane & 3;
    return ln;
}

// a use of a requested value that the compiler can neither move nor drop: the wait for the value stands HERE
template <class T> __device__ __forceinline__ void mlp_bwd_touch(const T x) { asm volatile("" :: "v"(x)); }

// ---------------------------------------------------------------------------------------------------------
// LDS
// ---------------------------------------------------------------------------------------------------------
// One object per workgroup; an instantiation holds only the parts of its mode, so the sizes are those of the separate arrays it
// replaces (float32 / bf16, bytes): wlds 11 040 + gtile 4 096 (+ beta_part 16 for rays) = 15 136 (15 152) with frozen decoders;
// + tiles 20 480 + ftile 17 408 / 9 216 + comb 21 824 = 74 848 (74 864) / 66 656 (66 672) with trainable ones.
//
//   wlds       per WORKGROUP.  Both decoders' weights (float32, or the bf16 image and its float32 biases).  Written by all 256
//              threads at the kernel's start (stage_decoder_weights[_lowp]), read by every lane's fragment load behind the
//              __syncthreads that follows; never written again.
//   gtile      per WAVE [pt][o].  The tile's output gradients: each lane writes its point's at the top of mlp_bwd_tile (sample role),
//              the contraction reads a block's 16 points of them (lanes r < 4).  The first WAVE_SYNC of the tile's first
//              block lies between; the tile's last WAVE_SYNC (end of its last block) lies between its last read and the
//              next tile's write.
//   tiles      per WAVE, WGRAD: gz1, gz2, h1, h2 of the block, written in the MFMA result layout (rows 4q+reg, column = point r),
//              read back as [point][row] by the contraction.  The block's first WAVE_SYNC separates write from read, its second
//              the read from the next block's write.
//   ftile      per WAVE, WGRAD: the block's features [pt][feature] (float32, or bf16 at half the pitch), written in the gather
//              role at the top of the block, read in the "feature on the lane" layout by the g_W1 contraction: the same two
//              WAVE_SYNCs as `tiles`.
//   beta_part  per WORKGROUP, rays: the four waves' sums of g_beta; lane 0 of each wave writes behind its last ray, thread 0
//              reads behind the __syncthreads of mlp_bwd_beta_partial.
//   comb       per WAVE, WGRAD: the wave's parameter gradients as a slab row, zeroed and (behind a WAVE_SYNC) written by
//              MlpBwdParamGrads::write_slab; the __syncthreads there separates the four waves' writes from the
//              workgroup's column sums.
struct MlpBwdLdsAll {
    __attribute__((aligned(16))) float wlds[2 * DEC_LDS];
    __attribute__((aligned(16))) float gtile[4][64 * 4];
};
template <bool LOWP> struct MlpBwdLdsWgrad {
    __attribute__((aligned(16))) float tiles[4][4][16 * TP];
    __attribute__((aligned(16))) float ftile[4][LOWP ? 16 * TPH / 2 : 16 * TPF];
    __attribute__((aligned(16))) float comb[4][SLAB];
};
struct MlpBwdLdsRays { float beta_part[4]; };
template <int> struct MlpBwdLdsNone {};            // (an empty base takes no room)
template <int MODE, bool WGRAD, bool LOWP>
struct MlpBwdLds : MlpBwdLdsAll, std::conditional_t<WGRAD, MlpBwdLdsWgrad<LOWP>, MlpBwdLdsNone<0>>,
                   std::conditional_t<MODE != 0, MlpBwdLdsRays, MlpBwdLdsNone<1>> {};

// ---------------------------------------------------------------------------------------------------------
// weight fragments: the transposed weights as A operands of the backward products (the forward fragment rebuilds the hidden layers)
// ---------------------------------------------------------------------------------------------------------
template <bool GZ> struct MlpBwdFragF32 {
    DecFrag f;
    float w3col[4], w2t[4], w1t[4][4];          // (w1t: not with GZ, which leaves W1^T . g_z1 to the scatter)

    __device__ __forceinline__ void load(const float* wlds, const MlpBwdLane& ln) {
        const float* L = wlds + ln.d * DEC_LDS;
        const int r = ln.r, q = ln.q;
        load_dec_frag(f, L, r, q);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            w3col[ks] = L[DEC_W3 + ks * 16 + r];                    // W3pad[o = ks][j = r]
            w2t[ks] = L[DEC_W2 + (4 * q + ks) * 16 + r];            // W2[j = 4q+ks][k' = r]
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)                          // row r of row block mb <-> feature (mb>>1)*32 + 16*(mb&1) + r:
                if (!GZ) w1t[mb][ks] = L[DEC_W1 + (4 * q + ks) * 64 + (mb >> 1) * 32 + 16 * (mb & 1) + r];   // lane q then holds piece q
        }
    }
};

struct MlpBwdFragBf16 {
    DecFragLP fl;
    short4_t w3colp = {0, 0, 0, 0}, w2tp = {0, 0, 0, 0}, w1tp[4];

    __device__ __forceinline__ void load(float* wlds, const MlpBwdLane& ln) {
        const int r = ln.r, q = ln.q;
        const short* W = lp_weights(wlds, ln.d);
        load_dec_frag_lp(fl, W, lp_biases(wlds, ln.d), r, q);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (q == 0) w3colp[jj] = W[LP_W3 + jj * 16 + r];                 // A[i = j = r][k = o = jj]: W3pad[o][j]
            w2tp[jj] = W[LP_W2 + (4 * q + jj) * 16 + r];                     // A[i = k' = r][k = j = 4q+jj]: W2[j][k']
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) w1tp[mb][jj] = W[LP_W1 + (4 * q + jj) * 64 + 16 * mb + r];   // W1[j][f = 16 mb + r]
        }
    }
};

template <bool LOWP, bool GZ> using MlpBwdFrag = std::conditional_t<LOWP, MlpBwdFragBf16, MlpBwdFragF32<GZ>>;

// ---------------------------------------------------------------------------------------------------------
// parameter-gradient accumulators (MFMA result layout) and the epilogue
// ---------------------------------------------------------------------------------------------------------
struct MlpBwdParamGrads {
    float4_t gW1[4], gW2, gW3, gb1, gb2;
    float gb3[3];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 4; ++i) gW1[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
        gW2 = gW3 = gb1 = gb2 = (float4_t){0.f, 0.f, 0.f, 0.f};
        gb3[0] = gb3[1] = gb3[2] = 0.f;
    }

    // the four waves' partial parameter gradients are summed in LDS; one slab row per workgroup: [wg][decoder][SLAB]
    __device__ __forceinline__ void write_slab(float (*comb)[SLAB], float* __restrict__ slabs, const MlpBwdLane& ln) const {
        const int lane = ln.lane, r = ln.r, q = ln.q;
        const int nout = ln.d ? 3 : 1;
        float* sl = comb[ln.wave];
        for (int i = lane; i < SLAB; i += WAVE) sl[i] = 0.0f;       // unwritten padding columns must not hold NaN bit patterns
        WAVE_SYNC();
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = 4 * q + reg;
            float4_t v;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) v[nb] = gW1[nb][reg];
            *(float4_t*)(sl + SL_W1 + j * 64 + 4 * r) = v;
            sl[SL_W2 + j * 16 + r] = gW2[reg];
            if (q == 0 && reg < nout) sl[SL_W3 + reg * 16 + r] = gW3[reg];
        }
        // bias gradients: sum over the 16 point lanes
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float a = gb1[reg], c = gb2[reg];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) {
                a += __shfl_xor(a, m, WAVE);
                c += __shfl_xor(c, m, WAVE);
            }
            if (r == 0) {
                sl[SL_B1 + 4 * q + reg] = a;
                sl[SL_B2 + 4 * q + reg] = c;
            }
        }
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float t = wave_sum(gb3[o]);
            if (lane == 0 && o < nout) sl[SL_B3 + o] = t;
        }
        __syncthreads();
        float* row = slabs + ((int64_t)blockIdx.x * 2 + ln.d) * SLAB;
        for (int col = threadIdx.x; col < SLAB; col += 256)     // columns no wave writes (padding) are never read back
            row[col] = (comb[0][col] + comb[1][col]) + (comb[2][col] + comb[3][col]);
    }
};

// ---------------------------------------------------------------------------------------------------------
// feature-gradient output
// ---------------------------------------------------------------------------------------------------------
// A wave's loads and stores retire in order on ONE counter (vmcnt).  A block's rows are requested a block ahead, i.e.
// BEFORE the previous block's four feature-gradient stores (GZ: its one g_z1 store; read 1 for 4 below), so "all but the 4
// youngest operations have retired" is all
// the top of a block has to wait for - but the compiler can only say so if it can COUNT the stores: as predicated
// global stores behind a branch (rows past the tile's end) it cannot, waits for vmcnt(0), and every block - and every
// ray's first use of its prefetched inputs - sat out the store acknowledgement of the block before (~2 k and ~5 k
// cycles: 45 % of a ray's ~30 k, profiles/r02/t_*).  The stores are therefore buffer stores that are ALWAYS issued - rows
// past the end get an offset beyond the descriptor's range, which the hardware drops - and four such dropped stores
// behind the first block's loads (issued by the drivers) give the block loop's entry the same shape as its back edge.
template <bool GZ> struct MlpBwdGradOut {
    typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned gz_base;              // GZ: where this decoder's g_z1 starts (bytes); 2 N * 64 < 2^32 - 256 follows from the launch's
                                   // check of N * 512
    int d, gp, gq;

    __device__ __forceinline__ MlpBwdGradOut(float* g_feat, int64_t N, const MlpBwdLane& ln)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc((void*)g_feat, 0, (int)((unsigned)N * (GZ ? 128u : 512u)), 0x00020000)),
          gz_base((unsigned)ln.d * ((unsigned)N * 64u)), d(ln.d), gp(ln.gp), gq(ln.gq) {}

    // as many stores as a block issues - four, GZ: one - that the hardware drops (offsets beyond the descriptor's range; distinct,
    // so that none is eliminated): they put "exactly four (GZ: one) stores are younger than every load issued before" into the
    // compiler's picture where a loop is entered
    __device__ __forceinline__ void dropped_stores() const {
#pragma unroll
        for (int j = 0; j < (GZ ? 1 : 4); ++j) __builtin_amdgcn_raw_buffer_store_b128((uint4_t){0u, 0u, 0u, 0u}, rsrc, (int)(0xFFFFFF00u + 16u * j), 0, 0);
    }
    // GZ: the block's g_z1 rows, gather role: lane (point gp, piece gq) holds hidden units 4gq..4gq+3, so a quad of lanes writes
    // one point's 64 contiguous bytes with ONE 16-byte store per lane, ALWAYS issued
    __device__ __forceinline__ void store_gz(const int64_t p0, const int b, const int nvalid, const float gzr[4]) const {
        const unsigned off = (16 * b + gp < nvalid) ? (unsigned)(p0 + 16 * b + gp) * 64u + gz_base + (unsigned)(gq * 16) : 0xFFFFFF00u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, (float4_t){gzr[0], gzr[1], gzr[2], gzr[3]}), rsrc, (int)off, 0, 0);
    }
    // the block's feature-gradient rows, gather role: four 16-byte stores per lane (both tiles: piece j at byte 64 j of the
    // decoder's half row), ALWAYS issued; N * 512 < 2^32 - 256 is checked at the launch
    __device__ __forceinline__ void store_rows(const int64_t p0, const int b, const int nvalid, const float gf[16]) const {
        const unsigned off = (16 * b + gp < nvalid) ? (unsigned)(p0 + 16 * b + gp) * 512u + (unsigned)(d * 256 + gq * 16) : 0xFFFFFF00u;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, (float4_t){gf[4 * j], gf[4 * j + 1], gf[4 * j + 2], gf[4 * j + 3]}),
                                                   rsrc, (int)off + 64 * j, 0, 0);
    }
};

// ---------------------------------------------------------------------------------------------------------
// one-block-ahead prefetch
// ---------------------------------------------------------------------------------------------------------
// fnext: the rows of the block that comes next - of this tile, or block 0 of the tile that comes next, requested by a tile's
// last block in front of its stores and waited for by the DRIVER (touch()) before it requests anything.
// hnext (SAVEDH): the saved h1 of the same block, requested at the same site; a block past the buffer's end - the wave has no
// further ray - is clamped, as rows past N are.
// ROWS: the block's feature rows are read at all (not with SAVEDH and frozen decoders).
// The type holds the values in flight and NOTHING else: with the pointers and the lane's indices beside them, five instantiations
// kept half of it on the stack (96 B of scratch, flat loads of the rows, vmcnt(0) round them).
template <bool LOWP, bool ROWS, bool SAVEDH> struct MlpBwdPrefetch {
    float4_t fnext[4];
    float4_t hnext = (float4_t){0.f, 0.f, 0.f, 0.f};

    // gather role: the 16 features of point pbase + gp, piece gq
    static __device__ __forceinline__ void load_block(const MlpBwdArgs& a, const MlpBwdLane& ln, float4_t v[4], const int64_t pbase) {
        const int64_t pt = min(pbase + ln.gp, a.N - 1);
        if (LOWP) {      // bf16 features (store_features_lp): channels 8gq..8gq+7 of each level, 16 bytes per level
            const short* fp = (const short*)a.feat + pt * 128 + ln.d * 64 + 8 * ln.gq;
            v[0] = *(const float4_t*)(fp);
            v[1] = *(const float4_t*)(fp + 32);
            v[2] = v[3] = (float4_t){0.f, 0.f, 0.f, 0.f};
            return;
        }
        const float* fp = a.feat + pt * 128 + ln.d * 64 + 4 * ln.gq;     // piece gq = channels 4gq.., 16+4gq.. of a level
        v[0] = *(const float4_t*)(fp);
        v[1] = *(const float4_t*)(fp + 16);
        v[2] = *(const float4_t*)(fp + 32);
        v[3] = *(const float4_t*)(fp + 48);
    }
    static __device__ __forceinline__ float4_t load_hidden(const MlpBwdArgs& a, const MlpBwdLane& ln, const int64_t hblk) {
        const int64_t hb_last = 2 * (int64_t)a.rb.R * hidden_blocks(a.rb.S) - 1;
        return *(const float4_t*)(a.hid + min(hblk, hb_last) * 256 + ln.lane * 4);
    }
    // the block whose rows start at point pbase and whose saved h1 is block hblk of `hid`
    __device__ __forceinline__ void request(const MlpBwdArgs& a, const MlpBwdLane& ln, const int64_t pbase, const int64_t hblk) {
        if (ROWS) load_block(a, ln, fnext, pbase);
        if (SAVEDH) hnext = load_hidden(a, ln, hblk);
    }
    __device__ __forceinline__ void touch() const {
        if (ROWS) { mlp_bwd_touch(fnext[0]); mlp_bwd_touch(fnext[1]); mlp_bwd_touch(fnext[2]); mlp_bwd_touch(fnext[3]); }
        if (SAVEDH) mlp_bwd_touch(hnext);
    }
};

// ---------------------------------------------------------------------------------------------------------
// one block of 16 points
// ---------------------------------------------------------------------------------------------------------
// What a block leaves for the weight-gradient contraction: the hidden layers and their pre-activation gradients, MFMA result
// layout (rows 4q+reg, column = point r)
struct MlpBwdBlockOut { float4_t h1, h2, gz1, gz2; };

// WGRAD: the block's results through LDS from the result layout to [point][row]; returns, for K = point 4q + ks of the
// contraction over the block's 16 points, the A operands az1, az2, ago and the B operands bh1, bh2
struct MlpBwdContract { float az1[4], az2[4], bh1[4], bh2[4], ago[4]; };
template <class Lds>
__device__ __forceinline__ MlpBwdContract mlp_bwd_transpose(Lds& lds, const MlpBwdLane& ln, const int b, const MlpBwdBlockOut& o) {
    const int r = ln.r, q = ln.q;
    float* tz1 = lds.tiles[ln.wave][0];
    float* tz2 = lds.tiles[ln.wave][1];
    float* th1 = lds.tiles[ln.wave][2];
    float* th2 = lds.tiles[ln.wave][3];
    const float* gt = lds.gtile[ln.wave];
    // transposes through LDS: D layout (rows 4q+reg, col = point r) -> [point][row]
    *(float4_t*)(tz1 + r * TP + 4 * q) = o.gz1;
    *(float4_t*)(tz2 + r * TP + 4 * q) = o.gz2;
    *(float4_t*)(th1 + r * TP + 4 * q) = o.h1;
    *(float4_t*)(th2 + r * TP + 4 * q) = o.h2;
    WAVE_SYNC();

    // parameter gradients: contraction over the block's 16 points (K = point 4q + ks)
    MlpBwdContract c;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int prow = 4 * q + ks;
        c.az1[ks] = tz1[prow * TP + r];
        c.az2[ks] = tz2[prow * TP + r];
        c.bh1[ks] = th1[prow * TP + r];
        c.bh2[ks] = th2[prow * TP + r];
        c.ago[ks] = (r < 4) ? gt[(16 * b + prow) * 4 + r] : 0.0f;
    }
    return c;
}

// ---- float32 ----
// the same rows again in the "feature on the lane" layout of the g_W1 contraction (B operand): NOT re-read from
// memory but handed over through a wave-private LDS tile, written here in the gather role and read back just before
// the contraction.  A global re-read (L1 / L2 hits) was waited for in the middle of the block - behind the previous
// block's four feature-gradient stores (GZ: one), a wave's loads and stores retiring in order - which exposed those stores'
// latency in every block (15 us of this kernel at 4096 x 64).
__device__ __forceinline__ void mlp_bwd_stage_rows_f32(float* ftile, const MlpBwdLane& ln, const float ft[16]) {
    float* T = ftile + ln.gp * TPF + 4 * ln.gq;
#pragma unroll
    for (int j = 0; j < 4; ++j) *(float4_t*)(T + 16 * j) = (float4_t){ft[4 * j], ft[4 * j + 1], ft[4 * j + 2], ft[4 * j + 3]};
}

// the hidden layers: h1 taken from the forward pass (SAVEDH) or rebuilt from the block's features, h2 recomputed
template <bool SAVEDH>
__device__ __forceinline__ void mlp_bwd_hidden_f32(const DecFrag& f, const float ft[16], const float4_t hsaved, float4_t& h1, float4_t& h2) {
    if (SAVEDH) { h1 = hsaved; mlp_hidden2(f, h1, h2); }
    else mlp_hidden(f, ft, h1, h2);
}

// backward through W3 and W2: go (sample role) -> g_z2, g_z1; the bias gradients take their sums
template <bool GZ>
__device__ __forceinline__ void mlp_bwd_w3_w2_f32(const MlpBwdFragF32<GZ>& w, const int q, const int b, const float go[4],
                                                  MlpBwdParamGrads& pg, MlpBwdBlockOut& o) {
    // g_h2^T = W3^T . g_o^T   (K = (block', o); only block' == b contributes)
    float4_t gh2 = (float4_t){0.f, 0.f, 0.f, 0.f};
    const bool mine = (q == b);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) gh2 = mfma16(mine ? w.w3col[ks] : 0.0f, go[ks], gh2);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.gz2[i] = o.h2[i] > 0.0f ? gh2[i] : 0.0f;
    // g_h1^T = W2^T . g_z2^T
    float4_t gh1 = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) gh1 = mfma16(w.w2t[ks], o.gz2[ks], gh1);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.gz1[i] = o.h1[i] > 0.0f ? gh1[i] : 0.0f;
    pg.gb1 += o.gz1;
    pg.gb2 += o.gz2;
}

// GZ: MFMA-role lane (r, q) holds rows 4q..4q+3 of point r: to the gather role, one store
__device__ __forceinline__ void mlp_bwd_store_gz1(const MlpBwdGradOut<true>& out, const int lane, const int64_t p0, const int b,
                                                  const int nvalid, const float4_t gz1) {
    float gzr[4] = {gz1[0], gz1[1], gz1[2], gz1[3]};
    to_gather_role<true, 4>(gzr, lane);
    out.store_gz(p0, b, nvalid, gzr);
}

// g_feat^T = W1^T . g_z1^T, four row blocks ordered so that MFMA-role lane (r, q) receives piece q of point r; row stores
__device__ __forceinline__ void mlp_bwd_w1_rows_f32(const MlpBwdFragF32<false>& w, const MlpBwdGradOut<false>& out, const int lane,
                                                    const int64_t p0, const int b, const int nvalid, const float4_t gz1) {
    float gf[16];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        float4_t acc = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc = mfma16(w.w1t[mb][ks], gz1[ks], acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) gf[(mb >> 1) * 8 + 4 * (mb & 1) + i] = acc[i];
    }
    to_gather_role<true, 16>(gf, lane);
    out.store_rows(p0, b, nvalid, gf);
}

// weight gradients: g_W2, g_W3 and g_W1 take the block's 16 points
template <class Lds>
__device__ __forceinline__ void mlp_bwd_wgrad_f32(Lds& lds, const MlpBwdLane& ln, const int b, const MlpBwdBlockOut& o,
                                                  MlpBwdParamGrads& pg) {
    const MlpBwdContract c = mlp_bwd_transpose(lds, ln, b, o);
    float4_t fbk[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        pg.gW2 = mfma16(c.az2[ks], c.bh1[ks], pg.gW2);              // g_W2[j][k'] : rows j = 4q+reg, col k' = r
        pg.gW3 = mfma16(c.ago[ks], c.bh2[ks], pg.gW3);              // g_W3[o][j]  : rows o = 4q+reg (q = 0), col j = r
    }
    // g_W1[j][f]: B = features of point 4q+ks, columns permuted: column c of n-block nb <-> feature 4c + nb
    // (the tile was written before this block's first WAVE_SYNC)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fbk[ks] = *(const float4_t*)(lds.ftile[ln.wave] + (4 * ln.q + ks) * TPF + 4 * ln.r);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) pg.gW1[nb] = mfma16(c.az1[ks], fbk[ks][nb], pg.gW1[nb]);
    }
    WAVE_SYNC();
}

// ft: the block's rows, gather role (ROWS); hsaved: its saved h1 (SAVEDH); go: the tile's output gradients, sample role
template <bool WGRAD, bool GZ, bool SAVEDH, class Lds>
__device__ __forceinline__ void mlp_bwd_block_f32(Lds& lds, const MlpBwdLane& ln, const MlpBwdFragF32<GZ>& w, MlpBwdParamGrads& pg,
                                                  const MlpBwdGradOut<GZ>& out, float ft[16], const float4_t hsaved, const float go[4],
                                                  const int64_t p0, const int b, const int nvalid) {
    if constexpr (WGRAD) mlp_bwd_stage_rows_f32(lds.ftile[ln.wave], ln, ft);
    if (!SAVEDH) to_mfma_role<true, 16>(ft, ln.lane);
    MlpBwdBlockOut o;
    mlp_bwd_hidden_f32<SAVEDH>(w.f, ft, hsaved, o.h1, o.h2);
    mlp_bwd_w3_w2_f32(w, ln.q, b, go, pg, o);
    if constexpr (GZ) mlp_bwd_store_gz1(out, ln.lane, p0, b, nvalid, o.gz1);
    else mlp_bwd_w1_rows_f32(w, out, ln.lane, p0, b, nvalid, o.gz1);
    if constexpr (WGRAD) mlp_bwd_wgrad_f32(lds, ln, b, o, pg);
}

// ---- bf16 (the mixed-precision tile of eslam_decode_tile.h): every product on bf16 MFMA with float32 accumulation ----
// the lane holds channels 8gq..8gq+7 of each level as 4 + 4 floats' worth of bits
__device__ __forceinline__ void mlp_bwd_stage_rows_bf16(float* ftile, const MlpBwdLane& ln, const float ft[16]) {
    short* T = (short*)ftile + ln.gp * TPH + 8 * ln.gq;
    *(float4_t*)(T) = (float4_t){ft[0], ft[1], ft[2], ft[3]};
    *(float4_t*)(T + 32) = (float4_t){ft[4], ft[5], ft[6], ft[7]};
}

// the hidden layers, recomputed from the block's bf16 features; a1, a2 are the pre-activations
__device__ __forceinline__ void mlp_bwd_hidden_bf16(const DecFragLP& fl, const float ft[16], float4_t& a1, float4_t& a2, float4_t& h1,
                                                    float4_t& h2) {
    short8_t bfeat[2];
#pragma unroll
    for (int lvl = 0; lvl < 2; ++lvl)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned u = __builtin_bit_cast(unsigned, ft[lvl * 4 + i]);
            bfeat[lvl][2 * i] = (short)(u & 0xFFFFu);
            bfeat[lvl][2 * i + 1] = (short)(u >> 16);
        }
    mlp_hidden_lp_bf(fl, bfeat, a1, a2);
#pragma unroll
    for (int i = 0; i < 4; ++i) { h1[i] = fmaxf(a1[i], 0.f); h2[i] = fmaxf(a2[i], 0.f); }
}

__device__ __forceinline__ void mlp_bwd_w3_w2_bf16(const MlpBwdFragBf16& w, const MlpBwdLane& ln, const int b, const float go[4],
                                                   const float4_t a1, const float4_t a2, MlpBwdParamGrads& pg, MlpBwdBlockOut& o) {
    const int r = ln.r, q = ln.q;
    const float4_t zero4 = (float4_t){0.f, 0.f, 0.f, 0.f};
    // g_h2^T = W3^T . g_o^T: B[k = o][col = point] lives on the q == 0 lanes; go is in sample role (lane = point of the tile)
    const float s0 = __shfl(go[0], 16 * b + r, WAVE), s1 = __shfl(go[1], 16 * b + r, WAVE), s2 = __shfl(go[2], 16 * b + r, WAVE);
    const short4_t bgo = (q == 0) ? pack4(s0, s1, s2, 0.f) : (short4_t){0, 0, 0, 0};
    const float4_t gh2 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w.w3colp, bgo, zero4, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.gz2[i] = a2[i] > 0.0f ? gh2[i] : 0.0f;
    const float4_t gh1 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w.w2tp, pack4(o.gz2[0], o.gz2[1], o.gz2[2], o.gz2[3]), zero4, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) o.gz1[i] = a1[i] > 0.0f ? gh1[i] : 0.0f;
    pg.gb1 += o.gz1;
    pg.gb2 += o.gz2;
}

// g_feat^T = W1^T . g_z1^T: row block mb = features 16 mb .. 16 mb + 15, lane (r, q) receives 16 mb + 4q + reg; row stores
__device__ __forceinline__ void mlp_bwd_w1_rows_bf16(const MlpBwdFragBf16& w, const MlpBwdGradOut<false>& out, const int lane,
                                                     const int64_t p0, const int b, const int nvalid, const float4_t gz1) {
    const float4_t zero4 = (float4_t){0.f, 0.f, 0.f, 0.f};
    float gf[16];
    const short4_t bz1 = pack4(gz1[0], gz1[1], gz1[2], gz1[3]);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const float4_t acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w.w1tp[mb], bz1, zero4, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) gf[4 * mb + i] = acc[i];
    }
    to_gather_role<true, 16>(gf, lane);
    out.store_rows(p0, b, nvalid, gf);
}

// the same contractions over the block's 16 points, K = 16 in one bf16 MFMA each
template <class Lds>
__device__ __forceinline__ void mlp_bwd_wgrad_bf16(Lds& lds, const MlpBwdLane& ln, const int b, const MlpBwdBlockOut& o,
                                                   MlpBwdParamGrads& pg) {
    const MlpBwdContract c = mlp_bwd_transpose(lds, ln, b, o);
    short4_t fbkp[4];
    pg.gW2 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pack4(c.az2[0], c.az2[1], c.az2[2], c.az2[3]),
                                                       pack4(c.bh1[0], c.bh1[1], c.bh1[2], c.bh1[3]), pg.gW2, 0, 0, 0);
    pg.gW3 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pack4(c.ago[0], c.ago[1], c.ago[2], c.ago[3]),
                                                       pack4(c.bh2[0], c.bh2[1], c.bh2[2], c.bh2[3]), pg.gW3, 0, 0, 0);
    const short4_t a1p = pack4(c.az1[0], c.az1[1], c.az1[2], c.az1[3]);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fbkp[ks] = *(const short4_t*)((const short*)lds.ftile[ln.wave] + (4 * ln.q + ks) * TPH + 4 * ln.r);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
        pg.gW1[nb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a1p, (short4_t){fbkp[0][nb], fbkp[1][nb], fbkp[2][nb], fbkp[3][nb]},
                                                               pg.gW1[nb], 0, 0, 0);
    WAVE_SYNC();
}

template <bool WGRAD, class Lds>
__device__ __forceinline__ void mlp_bwd_block_bf16(Lds& lds, const MlpBwdLane& ln, const MlpBwdFragBf16& w, MlpBwdParamGrads& pg,
                                                   const MlpBwdGradOut<false>& out, float ft[16], const float go[4], const int64_t p0,
                                                   const int b, const int nvalid) {
    if constexpr (WGRAD) mlp_bwd_stage_rows_bf16(lds.ftile[ln.wave], ln, ft);
    to_mfma_role<true, 8>(ft, ln.lane);       // 8 registers of packed bf16 pairs
    MlpBwdBlockOut o;
    float4_t a1, a2;
    mlp_bwd_hidden_bf16(w.fl, ft, a1, a2, o.h1, o.h2);
    mlp_bwd_w3_w2_bf16(w, ln, b, go, a1, a2, pg, o);
    mlp_bwd_w1_rows_bf16(w, out, ln.lane, p0, b, nvalid, o.gz1);
    if constexpr (WGRAD) mlp_bwd_wgrad_bf16(lds, ln, b, o, pg);
}

// ---------------------------------------------------------------------------------------------------------
// one tile of <= 64 points
// ---------------------------------------------------------------------------------------------------------
// MLP backward of the tile starting at point p0; go[] = this decoder's pre-activation output gradients of the lane's point
// (sample role).  The tile's first block has been requested (pf); its last block requests block 0 of the tile at p0_next.
// hb: the tile's first block in `hid`, hb_next that of the tile that comes next (SAVEDH).
template <bool WGRAD, bool LOWP, bool GZ, bool SAVEDH, class Lds, class Prefetch>
__device__ __forceinline__ void mlp_bwd_tile(const MlpBwdArgs& a, Lds& lds, const MlpBwdLane& ln, const MlpBwdFrag<LOWP, GZ>& w, MlpBwdParamGrads& pg,
                                             const MlpBwdGradOut<GZ>& out, Prefetch& pf, const int64_t p0, const int nvalid,
                                             const float go[4], const int64_t p0_next, const int64_t hb, const int64_t hb_next) {
    constexpr bool ROWS = !SAVEDH || WGRAD;
    const int nblk = (nvalid + 15) >> 4;
    __builtin_assume(nblk >= 1);
#pragma unroll
    for (int o = 0; o < 3; ++o) pg.gb3[o] += go[o];
    *(float4_t*)(lds.gtile[ln.wave] + ln.lane * 4) = (float4_t){go[0], go[1], go[2], go[3]};

    // The rows of block b+1 are requested before block b is computed: at 2 waves per SIMD nothing else hides the ~2k-cycle load
    // latency.  (MlpBwdGradOut: why the top of a block then waits for all but the youngest four operations, and no longer.)
#pragma unroll 1
    for (int b = 0; b < nblk; ++b) {
        float ft[16];
        if (ROWS) {
            const float4_t f0 = pf.fnext[0], f1 = pf.fnext[1], f2 = pf.fnext[2], f3 = pf.fnext[3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ft[i] = f0[i]; ft[4 + i] = f1[i]; ft[8 + i] = f2[i]; ft[12 + i] = f3[i];
            }
        }
        const float4_t hsaved = pf.hnext;
        // (two blocks ahead: 250 VGPRs, no faster.)  ONE request site with a selected address: two sites behind an if / else
        // made the compiler wait for vmcnt(0)
        pf.request(a, ln, b + 1 < nblk ? p0 + 16 * (b + 1) : p0_next, b + 1 < nblk ? hb + b + 1 : hb_next);
        if constexpr (LOWP) mlp_bwd_block_bf16<WGRAD>(lds, ln, w, pg, out, ft, go, p0, b, nvalid);
        else mlp_bwd_block_f32<WGRAD, GZ, SAVEDH>(lds, ln, w, pg, out, ft, hsaved, go, p0, b, nvalid);
    }
}

// ---------------------------------------------------------------------------------------------------------
// MODE 0: tiles of 64 free points, pre-activation output gradients g_o [N,4] from memory (decode_act_bwd_kernel)
// ---------------------------------------------------------------------------------------------------------
template <bool WGRAD, bool LOWP, class Lds, class Prefetch>
__device__ __forceinline__ void mlp_bwd_points(const MlpBwdArgs& a, Lds& lds, const MlpBwdLane& ln, const MlpBwdFrag<LOWP, false>& w,
                                               MlpBwdParamGrads& pg, const MlpBwdGradOut<false>& out, Prefetch& pf) {
    const int64_t N = a.N;
    const int64_t ntiles = (N + 63) / 64;
    int64_t tile = (int64_t)blockIdx.x * 4 + ln.wave;
    if (tile < ntiles) {
        pf.request(a, ln, tile * 64, 0);
        out.dropped_stores();
    }
    for (; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t p0 = tile * 64;
        const int nvalid = (int)min((int64_t)64, N - p0);
        // sample role: pre-activation output gradients of this decoder
        float go[4] = {0.f, 0.f, 0.f, 0.f};
        if (ln.lane < nvalid) {
            const float4_t g = *(const float4_t*)(a.g_o + (p0 + ln.lane) * 4);
            if (ln.d == 0) go[0] = g[3];
            else { go[0] = g[0]; go[1] = g[1]; go[2] = g[2]; }
        }
        pf.touch();
        mlp_bwd_tile<WGRAD, LOWP, false, false>(a, lds, ln, w, pg, out, pf, p0, nvalid, go, (tile + (int64_t)gridDim.x * 4) * 64, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// MODE 1, 2: a wave owns a ray
// ---------------------------------------------------------------------------------------------------------
// What the composite backward of a ray reads is REQUESTED ONE RAY AHEAD: a persistent wave walks its rays one after the
// other, and a load -> scan -> decoder chain per ray put ~2.5 us of exposed latency in front of every ray's MFMAs
// (8192 x 96: 228 us fused against 208 us for the three launches it replaced).  A wave's loads retire in issue
// order, so the prefetched values have arrived by the time the current ray's later feature loads are waited for.
struct RayIn {                     // a ray's scalars: upstream gradients, and (MODE 2) what the loss gradient reads
    float gd, gr, gg, gb, gtd, dep, cr, cg, cb, tr, tg, tb;
    int mask;

    template <int MODE> static __device__ __forceinline__ RayIn load(const RayBwdIn& rb, const LossGradIn& li, int ray) {
        RayIn x;
        x.gd = rb.g_depth ? rb.g_depth[ray] : 0.0f;
        x.gr = rb.g_rgb ? rb.g_rgb[3 * ray + 0] : 0.0f;
        x.gg = rb.g_rgb ? rb.g_rgb[3 * ray + 1] : 0.0f;
        x.gb = rb.g_rgb ? rb.g_rgb[3 * ray + 2] : 0.0f;
        x.gtd = x.dep = x.cr = x.cg = x.cb = x.tr = x.tg = x.tb = 0.0f;
        x.mask = 1;
        if (MODE == 2) {
            x.gtd = li.gt_depth[ray];
            x.mask = li.ray_mask ? (int)li.ray_mask[ray] : 1;      // the byte as loaded: comparing it here would wait for it here
            x.dep = li.depth[ray];
            x.cr = li.rgb[3 * ray + 0]; x.cg = li.rgb[3 * ray + 1]; x.cb = li.rgb[3 * ray + 2];
            x.tr = li.gt_color[3 * ray + 0]; x.tg = li.gt_color[3 * ray + 1]; x.tb = li.gt_color[3 * ray + 2];
        }
        return x;
    }
    __device__ __forceinline__ void touch() const {
        mlp_bwd_touch(gd); mlp_bwd_touch(gr); mlp_bwd_touch(gg); mlp_bwd_touch(gb); mlp_bwd_touch(gtd); mlp_bwd_touch(dep);
        mlp_bwd_touch(cr); mlp_bwd_touch(cg); mlp_bwd_touch(cb); mlp_bwd_touch(tr); mlp_bwd_touch(tg); mlp_bwd_touch(tb);
        mlp_bwd_touch(mask);
    }
};

struct ChunkIn {                   // 64 samples of a ray, sample role
    float sd, z, cr, cg, cb, gs;

    static __device__ __forceinline__ ChunkIn load(const RayBwdIn& rb, int ray, int c, int lane) {
        ChunkIn x = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int S = rb.S;
        const int s = c * WAVE + lane;
        if (s < S) {
            const int64_t i = (int64_t)ray * S + s;
            x.sd = rb.sdf[i];
            x.z = rb.z_vals[i];
            x.cr = rb.raw_rgb[i * 3 + 0];
            x.cg = rb.raw_rgb[i * 3 + 1];
            x.cb = rb.raw_rgb[i * 3 + 2];
            if (rb.g_sdf) x.gs = rb.g_sdf[i];
        }
        return x;
    }
    __device__ __forceinline__ void touch() const {
        mlp_bwd_touch(sd); mlp_bwd_touch(z); mlp_bwd_touch(cr); mlp_bwd_touch(cg); mlp_bwd_touch(cb); mlp_bwd_touch(gs);
    }
};

// S > 64: the sdf values of the chunks in front of the last one (ray_pass_a), requested a ray ahead like the rest
static_assert(ESLAM_MAX_SAMPLES <= 4 * WAVE, "pass A prefetch holds three chunks");
struct PassA {
    float sd[3];

    static __device__ __forceinline__ PassA load(const RayBwdIn& rb, int ray, int nchunk, int lane) {
        PassA x = {{0.f, 0.f, 0.f}};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < nchunk - 1) x.sd[k] = rb.sdf[(int64_t)ray * rb.S + k * WAVE + lane];      // chunks before the last are full
        return x;
    }
    __device__ __forceinline__ void touch() const { mlp_bwd_touch(sd[0]); mlp_bwd_touch(sd[1]); mlp_bwd_touch(sd[2]); }
};

// MODE 2: the gradient of the mapping loss (src/Mapper.py:110-144,337-346) from the global set sizes in li.acc - the factors
// once per wave, a ray's upstream values per ray.  MODE 1: the upstream values are those of memory alone.
template <int MODE> struct RayLossGrad {
    LossW lw = {};
    LossK lk = {};
    float nd = 1.0f, ncol = 1.0f;

    __device__ __forceinline__ explicit RayLossGrad(const LossGradIn& li) {
        if (MODE == 2) {
            lw = loss_scaled_weights(li.w, li.upstream);
            lk = loss_sdf_factors(lw, li.tr, li.acc);
            nd = li.acc[A_N_DEPTH]; ncol = li.acc[A_N_COLOR];
            if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && li.loss_out)
                li.loss_out[0] = loss_value_from_acc(li.w, li.acc);
        }
    }
    // d L / d (depth, rgb) of the ray; m: the ray is in the loss's depth set (its sdf terms count).  Filled in place, not returned:
    // a RayUp returned by value is copied as a block, gr and gg are then paired into packed multiply + add where two fused
    // multiply-adds stood, and every gradient of the fused loss changes in its last bits
    __device__ __forceinline__ void upstream(const RayIn& rin, RayUp& up, bool& m) const {
        up.gd = rin.gd; up.gr = rin.gr; up.gg = rin.gg; up.gb = rin.gb;
        m = false;
        if (MODE == 2) {
            const bool mc = rin.mask != 0;
            m = mc && rin.gtd > 0.0f;
            up.gd += loss_g_depth(m, rin.gtd, rin.dep, lw, nd);
            up.gr += loss_g_color(mc, rin.tr, rin.cr, lw, ncol);
            up.gg += loss_g_color(mc, rin.tg, rin.cg, lw, ncol);
            up.gb += loss_g_color(mc, rin.tb, rin.cb, lw, ncol);
        }
    }
};

// pass A: transmittance product of every chunk; lane c keeps chunk c's
__device__ __forceinline__ float ray_pass_a(const PassA& pin, const float beta, const int nchunk, const int lane) {
    float myprod = 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                    // (the last chunk's product is never needed)
        if (c < nchunk - 1) {
            const float sd = pin.sd[c];
            const float alpha = 1.0f - expf(-beta * sigmoidf_(-sd * beta));
            const float cp = wave_lane<63>(wave_incl_prod((1.0f - alpha) + 1e-10f, lane));
            if (lane == c) myprod = cp;
        }
    }
    return myprod;
}

// where chunk c of a ray's saved h1 starts in `hid` (blocks of 16 samples; SB = hidden_blocks(S) per ray; chunk c starts at block 4 c)
__device__ __forceinline__ int64_t ray_hidden_block(int d, int R, int64_t SB, int ray, int c) { return ((int64_t)d * R + ray) * SB + 4 * c; }

// The wave runs the composite backward of its rays' chunks (upstream gradients from memory, MODE 2: plus the loss's) and feeds
// the result to the MLP backward from registers - the sample role of the one IS the B operand of the other.  Both decoders'
// workgroups (blockIdx.y) repeat the scalar composite work.  Returns the lane's part of g_beta.
template <int MODE, bool WGRAD, bool LOWP, bool GZ, bool SAVEDH, class Lds, class Prefetch>
__device__ __forceinline__ float mlp_bwd_rays(const MlpBwdArgs& a, Lds& lds, const MlpBwdLane& ln, const MlpBwdFrag<LOWP, GZ>& w,
                                              MlpBwdParamGrads& pg, const MlpBwdGradOut<GZ>& out, Prefetch& pf) {
    const RayBwdIn& rb = a.rb;
    const LossGradIn& li = a.li;
    const int lane = ln.lane, d = ln.d;
    const int R = rb.R, S = rb.S;
    const int nchunk = (S + WAVE - 1) / WAVE;
    const int64_t SB = hidden_blocks(S);
    __builtin_assume(nchunk >= 1);             // (S >= 1 is checked at the launch; lets the compiler count a ray's stores)
    const float beta = rb.beta[0];
    const RayLossGrad<MODE> loss(li);
    float gbeta_acc = 0.0f;
    const int stride = gridDim.x * 4;
    int ray = blockIdx.x * 4 + ln.wave;
    RayIn rin = {};
    ChunkIn cin = {};
    PassA pin = {{0.f, 0.f, 0.f}};
    if (ray < R) {
        rin = RayIn::load<MODE>(rb, li, ray);
        cin = ChunkIn::load(rb, ray, nchunk - 1, lane);
        pin = PassA::load(rb, ray, nchunk, lane);
        pf.request(a, ln, (int64_t)ray * S + (nchunk - 1) * WAVE, ray_hidden_block(d, R, SB, ray, nchunk - 1));
    }
    out.dropped_stores();                                     // the waits below are counted by the compiler: see MlpBwdGradOut
    for (; ray < R; ray += stride) {
        const int64_t base = (int64_t)ray * S;
        // What is requested ahead - this ray's scalars and its last chunk a ray ago, a further chunk a tile ago - is waited
        // for HERE, in front of the next requests and behind the four stores that ended the tile in between: vmcnt(4)
        // (GZ: one store, vmcnt(1)).
        // (Waited for at its first use further down, the wait would cover the requests issued meanwhile as well - the
        // compiler cannot count those: optional pointers, rows past S - and expose their whole latency in every ray:
        // 5.5 k cycles of a ray's ~30 k, profiles/r02/t_*.)
        rin.touch();
        cin.touch();
        pin.touch();
        pf.touch();
        ChunkIn ch = cin;
        RayIn rnx = {};
        ChunkIn cnx = {};
        PassA pnx = {{0.f, 0.f, 0.f}};
        if (ray + stride < R) {
            rnx = RayIn::load<MODE>(rb, li, ray + stride);
            cnx = ChunkIn::load(rb, ray + stride, nchunk - 1, lane);
            pnx = PassA::load(rb, ray + stride, nchunk, lane);
        }
        RayUp up;
        bool m;
        loss.upstream(rin, up, m);
        const float gtd = rin.gtd;
        const float myprod = ray_pass_a(pin, beta, nchunk, lane);
        // pass B: chunks in reverse, carrying the suffix sum of gw*w
        float carry = 0.0f;
        int c = nchunk - 1;
        do {
            // S > 64: the chunk in front of this one is requested a tile ahead as well, and taken over behind the tile's stores.
            // (No value still in flight is carried around a loop: the compiler copies loop-carried registers at the loop's
            // entry, and a copy of a register that is still being loaded is a wait for everything requested so far.)
            ChunkIn cn = {};
            if (c > 0) cn = ChunkIn::load(rb, ray, c - 1, lane);
            float trans_in = 1.0f;
            for (int k = 0; k < c; ++k) trans_in *= __shfl(myprod, k, WAVE);
            const bool valid = c * WAVE + lane < S;
            float gs = ch.gs;
            if (MODE == 2 && valid) gs += loss_g_sdf(m, ch.z, ch.sd, gtd, li.tr, loss.lk);
            const float4_t o = composite_bwd_chunk(up, beta, valid, ch.sd, ch.z, ch.cr, ch.cg, ch.cb, gs, trans_in, carry,
                                                   gbeta_acc, lane);
            float go[4] = {0.f, 0.f, 0.f, 0.f};
            if (d == 0) go[0] = o[3];
            else { go[0] = o[0]; go[1] = o[1]; go[2] = o[2]; }
            // the tile after this one: the chunk in front of it, or the last chunk of the wave's next ray (rows past N are clamped)
            mlp_bwd_tile<WGRAD, LOWP, GZ, SAVEDH>(a, lds, ln, w, pg, out, pf, base + c * WAVE, min(WAVE, S - c * WAVE), go,
                                                  c > 0 ? base + (c - 1) * WAVE : (int64_t)(ray + stride) * S + (nchunk - 1) * WAVE,
                                                  ray_hidden_block(d, R, SB, ray, c),
                                                  c > 0 ? ray_hidden_block(d, R, SB, ray, c - 1) : ray_hidden_block(d, R, SB, ray + stride, nchunk - 1));
            if (c > 0) {
                cn.touch();
                pf.touch();
                ch = cn;
            }
        } while (--c >= 0);
        rin = rnx;
        cin = cnx;
        pin = pnx;
    }
    return gbeta_acc;
}

// g_beta: one partial sum per workgroup of the sdf decoder (summed by dec_grad_reduce_kernel / beta_sum_kernel);
// one atomic per ray on the single address of g_beta would serialise at the memory side (4096 of them: 50 us)
__device__ __forceinline__ void mlp_bwd_beta_partial(float* beta_part, float* beta_parts, const float gbeta_acc, const MlpBwdLane& ln) {
    const float tot = wave_sum(gbeta_acc);
    if (ln.lane == 0) beta_part[ln.wave] = tot;
    __syncthreads();
    if (ln.d == 0 && threadIdx.x == 0 && beta_parts)
        beta_parts[blockIdx.x] = (beta_part[0] + beta_part[1]) + (beta_part[2] + beta_part[3]);
}
