// Forward kernels: fused tri-plane gather -> SDF/colour MLPs -> volumetric composite (render), and the
// decoder-only variant on free points (Decoders.forward / get_raw_sdf).
//
// One wave64 = one ray (render) or one tile of 64 points (decode); 4 waves per workgroup share an LDS copy of
// the decoder weights.  See eslam_decode_tile.h for the lane roles and the MFMA operand plan.
#include "eslam_decode_tile.h"
#include "eslam_loss_final.h"

// ---------------------------------------------------------------------------------------------------------
// render: replaces reference src/utils/Renderer.py:136-147 (+ decoders.py:64-146, common.py:204-218)
// ---------------------------------------------------------------------------------------------------------
// LOSS: the kernel also forms the sums of the callers' loss (src/Mapper.py:110-144,337-346) from the values it has in
// registers anyway - per sample the region of z against gt_depth and the squared SDF error, per ray the depth and colour
// errors - reduces them per workgroup and finishes acc [16] and the loss value with the ticket scheme of eslam_loss_value:
// one launch less per iteration (14 us), and sdf / depth / rgb are not read back for it.
struct LossIn {
    const float* gt_depth;
    const float* gt_color;
    const uint8_t* ray_mask;
    float* scratch;
    float* acc;
    float* loss;
    Trunc tr;
    LossW w;
    int det;               // ESLAM_DETERMINISTIC: fixed-order reduction of the workgroups' sums
};

#define FWD_WAVES 2            // waves per SIMD the gather kernels are compiled for: with one plane of loads in flight
                               // ahead of the FMAs the forward kernel needs 195 VGPRs; 2 waves/SIMD measured fastest

// The mixed-precision decode kernels on free points (decode_fwd_kernel<true, ..., true>), none with scratch: SDF only 124
// VGPRs (list and grid), both fields 126 - 4 waves per SIMD; both fields with saved features 140 - 3 waves.  Asked for 4
// waves (128 VGPRs) the saving variant spills 40 bytes per lane, so 3 is what is asked and the others take 4 on their own.
#define DECODE_LP_WAVES 3

// LOWP: the mixed-precision tile of eslam_decode_tile.h (fp16 plane copies, bf16 MFMA decoders); channels-last only.
template <bool CL, bool SAVE, bool LOSS, bool LOWP>
__global__ __launch_bounds__(256, FWD_WAVES) void render_fwd_kernel(const PlaneSet planes, const eslam_decoders_t dec,
                                                         const Bound bnd, const float* __restrict__ rays_o,
                                                         const float* __restrict__ rays_d,
                                                         const float* __restrict__ z_vals, int R, int S,
                                                         float* __restrict__ depth_out, float* __restrict__ rgb_out,
                                                         float* __restrict__ sdf_out, float* __restrict__ raw_rgb_out,
                                                         float* __restrict__ feat_out, float* __restrict__ hid_out,
                                                         const int* __restrict__ perm, const LossIn li,
                                                         uint32_t* __restrict__ rng_bump) {
    // the samplers drew this iteration's random numbers from (seed, *rng_bump) before this kernel started
    // (eslam_sample_z_all_rng): advance the step for the next iteration (of a replayed graph)
    if (rng_bump && blockIdx.x == 0 && threadIdx.x == 0) rng_bump[0] += 1u;
    __shared__ __attribute__((aligned(16))) float wlds[2 * DEC_LDS];
    static_assert(LP_LDS_FLOATS <= 2 * DEC_LDS, "the bf16 weight image shares the float32 image's LDS");
    if (LOWP) stage_decoder_weights_lowp(wlds, dec, threadIdx.x, blockDim.x);
    else stage_decoder_weights(wlds, dec, threadIdx.x, blockDim.x);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;                                  // MFMA role
    const int gp = gather_point<CL>(lane), gq = gather_piece<CL>(lane);     // gather role
    // (R * S * 512 < 2^32 - 256 is checked at the launch when features are saved)
    const __amdgpu_buffer_rsrc_t frsrc = __builtin_amdgcn_make_buffer_rsrc((void*)feat_out, 0, (int)((unsigned)R * (unsigned)S * 512u), 0x00020000);
    // the saved first hidden layer (float32 planes, SAVE): 2 R SB blocks of 1 KB, checked at the launch as well; no buffer given =
    // a descriptor of zero length, whose stores the hardware drops
    const int SB = (int)hidden_blocks(S);
    const __amdgpu_buffer_rsrc_t hrsrc = __builtin_amdgcn_make_buffer_rsrc((void*)hid_out, 0, hid_out ? (int)(2u * (unsigned)R * (unsigned)SB * 1024u) : 0, 0x00020000);
    float lv[A_COUNT];                     // LOSS: this lane's share of the accumulators
#pragma unroll
    for (int k = 0; k < A_COUNT; ++k) lv[k] = 0.0f;
    // Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one, MI355X_MICROARCH.md).  Give every
    // XCD a contiguous run of the ray order, so that rays through neighbouring pixels - which read the same texels -
    // are resident on CUs behind the same L2.  Placement only affects speed: the grid has 8*cpx blocks, every logical
    // block is taken exactly once, surplus blocks exit.
    const int cpx = gridDim.x >> 3;
    const int lblock = (blockIdx.x & 7) * cpx + (blockIdx.x >> 3);
    if (!LOSS && lblock * 4 + wave >= R) return;
    // Persistent over the rays when the batch has more workgroups' worth of rays than the chip holds at once (the host caps the
    // grid at FWD_WAVES workgroups per CU): the decoder weights are staged once per resident workgroup instead of once per
    // four rays.  Round k gives every XCD the next contiguous run of the ray order.
    // (LOSS: idle waves still take part in the workgroup's reduction below)
    for (int slot = lblock * 4 + wave; slot < R; slot += (int)gridDim.x * 4) {
    const int ray = perm ? perm[slot] : slot;
    const float gtd = LOSS ? li.gt_depth[ray] : 0.0f;
    const bool in_batch = LOSS ? (li.ray_mask ? li.ray_mask[ray] != 0 : true) : false;
    const bool has_depth = in_batch && gtd > 0.0f;

    const float ox = rays_o[ray * 3 + 0], oy = rays_o[ray * 3 + 1], oz = rays_o[ray * 3 + 2];
    const float dx = rays_d[ray * 3 + 0], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
    const float beta = dec.beta[0];
    const float* zrow = z_vals + (int64_t)ray * S;

    float trans_in = 1.0f;                 // transmittance entering the chunk
    float acc_depth = 0.0f, acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;

    for (int c0 = 0; c0 < S; c0 += WAVE) {
        const int nvalid = min(WAVE, S - c0);
        const int nblk = (nvalid + 15) >> 4;

        float4_t out[2];
        // gather role: normalised coordinates of point 16b + gp of the chunk
        // the chunk's z values, sample role (lane l: sample min(c0 + l, S - 1)); a block's points fetch theirs with a lane
        // permute - as a load per block the value sat on the critical path of the NEXT block's first texel request
        const float zs = zrow[min(c0 + lane, S - 1)];
        auto block_point = [&](int b, float& px, float& py, float& pz) {
            const float zb = __shfl(zs, 16 * b + gp, WAVE);
            px = norm_coord(ox + dx * zb, bnd.lo[0], bnd.hi[0]);
            py = norm_coord(oy + dy * zb, bnd.lo[1], bnd.hi[1]);
            pz = norm_coord(oz + dz * zb, bnd.lo[2], bnd.hi[2]);
        };
        constexpr bool CHAIN = CL && !LOWP;    // float32 channels-last planes: texel requests run one block ahead
        PlaneTaps carry;
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (CHAIN) {
            block_point(0, cx, cy, cz);
            issue_plane0(planes, 0, cx, cy, cz, gq, opaque_zero(c0), carry);
        }
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            out[d] = LOWP ? *(const float4_t*)(lp_biases(wlds, d) + 32) : *(const float4_t*)(wlds + d * DEC_LDS + DEC_B3);
#pragma unroll 1
            for (int b = 0; b < nblk; ++b) {
                const int oz0 = opaque_zero(b);
                const int sb = c0 + 16 * b + gp;
                float feat[16];
                if (CHAIN) {
                    const bool last = b + 1 == nblk;
                    float nx, ny, nz;
                    block_point(last ? 0 : b + 1, nx, ny, nz);
                    gather_features_chain(planes, d, cx, cy, cz, gq, feat, oz0, carry, last ? 1 : d, nx, ny, nz);
                    cx = nx; cy = ny; cz = nz;
                    if (SAVE) {
                        // the saved features leave through always-issued buffer stores (countable: store_features_buffer)
                        __builtin_amdgcn_sched_barrier(0);      // (left alone, the scheduler sinks the stores behind the MLP)
                        store_features_buffer(frsrc, sb < S ? (unsigned)(ray * S + sb) * 512u + (unsigned)(d * 256 + gq * 16)
                                                            : ESLAM_OOB_OFFSET, feat);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    to_mfma_role<CL, 16>(feat, lane);
                    DecFrag f;
                    load_dec_frag(f, wlds + d * DEC_LDS + oz0, r, q);
                    float4_t h1, h2;
                    mlp_hidden(f, feat, h1, h2);
                    if (SAVE) store_hidden_buffer(hrsrc, (unsigned)((d * R + ray) * SB + (c0 >> 4) + b) * 1024u + (unsigned)lane * 16u, h1);
                    mlp_out_accum(f, h2, b, r, out[d]);
                    continue;
                }
                float px, py, pz;
                block_point(b, px, py, pz);
                if (LOWP) {
                    gather_features_half(planes, d, px, py, pz, gq, feat, oz0);
                    if (SAVE) {
                        if (sb < S) store_features_lp(feat_out, (int64_t)ray * S + sb, d, gq, feat);
                    }
                    to_mfma_role<true, 16>(feat, lane);
                    DecFragLP fl;
                    load_dec_frag_lp(fl, lp_weights(wlds, d) + oz0, lp_biases(wlds, d) + oz0, r, q);
                    float4_t a1, a2;
                    mlp_hidden_lp(fl, feat, a1, a2);
                    mlp_out_accum_lp(fl, a2, b, r, out[d]);
                    continue;
                }
                gather_features<CL>(planes, d, px, py, pz, gq, feat, oz0);
                if (SAVE) {
                    if (sb < S) store_features(feat_out, (int64_t)ray * S + sb, d, gq, feat);
                }
                to_mfma_role<CL, 16>(feat, lane);
                // operand fragments are re-read from LDS per block (9 ds_read_b128) instead of being kept live across
                // the gather, where they would push the kernel past 128 VGPRs
                DecFrag f;
                load_dec_frag(f, wlds + d * DEC_LDS + oz0, r, q);
                float4_t h1, h2;
                mlp_hidden(f, feat, h1, h2);
                if (SAVE) store_hidden_buffer(hrsrc, (unsigned)((d * R + ray) * SB + (c0 >> 4) + b) * 1024u + (unsigned)lane * 16u, h1);
                mlp_out_accum(f, h2, b, r, out[d]);
            }
        }

        // ---- sample role: activations, alpha, transmittance scan, composite (Renderer.py:140-153) ----
        const bool valid = lane < nvalid;
        const int s = c0 + lane;
        const float z = valid ? zs : 0.0f;
        const float sdf = tanhf(out[0][0]);
        const float cr = sigmoidf_(out[1][0]), cg = sigmoidf_(out[1][1]), cb = sigmoidf_(out[1][2]);
        if (valid) {
            sdf_out[(int64_t)ray * S + s] = sdf;
            if (SAVE) {
                float* rr = raw_rgb_out + ((int64_t)ray * S + s) * 3;
                rr[0] = cr; rr[1] = cg; rr[2] = cb;
            }
        }
        const float sg = sigmoidf_(-sdf * beta);
        float alpha = 1.0f - expf(-beta * sg);
        if (!valid) alpha = 0.0f;
        const float fac = valid ? (1.0f - alpha) + 1e-10f : 1.0f;
        const float pin = wave_incl_prod(fac, lane);
        const float pex = wave_up1(pin, 1.0f);
        const float w = alpha * (trans_in * pex);
        acc_depth += wave_sum(w * z);
        acc_r += wave_sum(w * cr);
        acc_g += wave_sum(w * cg);
        acc_b += wave_sum(w * cb);
        trans_in *= wave_lane<63>(pin);
        if (LOSS && valid && has_depth) {              // Mapper.py:124-140
            const int reg = sdf_region(z, gtd, li.tr);
            if (reg == 0) { lv[A_N_FRONT] += 1.0f; const float e = sdf - 1.0f; lv[A_S_FRONT] += e * e; }
            else if (reg == 1) { lv[A_N_CENTER] += 1.0f; const float e = (z + sdf * li.tr.t) - gtd; lv[A_S_CENTER] += e * e; }
            else if (reg == 2) { lv[A_N_TAIL] += 1.0f; const float e = (z + sdf * li.tr.t) - gtd; lv[A_S_TAIL] += e * e; }
        }
    }
    if (lane == 0) {
        depth_out[ray] = acc_depth;
        rgb_out[ray * 3 + 0] = acc_r;
        rgb_out[ray * 3 + 1] = acc_g;
        rgb_out[ray * 3 + 2] = acc_b;
        if (LOSS) {                                    // Mapper.py:343,346
            if (has_depth) { const float e = gtd - acc_depth; lv[A_N_DEPTH] += 1.0f; lv[A_S_DEPTH] += e * e; }
            if (in_batch) {
                const float er = li.gt_color[3 * ray] - acc_r, eg = li.gt_color[3 * ray + 1] - acc_g,
                            eb = li.gt_color[3 * ray + 2] - acc_b;
                lv[A_S_COLOR] += (er * er + eg * eg) + eb * eb;
                lv[A_N_COLOR] += 3.0f;
            }
        }
    }
    }
    if (LOSS) {
        __shared__ float red[4][A_COUNT];
#pragma unroll
        for (int k = 0; k < A_COUNT; ++k) {
            const float t = wave_sum(lv[k]);
            if (lane == 0) red[wave][k] = t;
        }
        __syncthreads();
        float tot = 0.0f;
        if (threadIdx.x < A_COUNT)
            tot = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (li.det) loss_finalize_det(tot, li.scratch, li.acc, li.w, li.loss);
        else loss_finalize(tot, li.scratch, li.acc, li.w, li.loss);
    }
}

// ---------------------------------------------------------------------------------------------------------
// decode on free points: replaces reference src/networks/decoders.py:127-146 (and :87-105 when SDF_ONLY)
// ---------------------------------------------------------------------------------------------------------
// Point sources of decode_fwd_kernel.  A source cuts its points into wave tiles of at most 64 consecutive output
// indices, gives each point's world coordinates, and may classify a whole tile against a convex region.
enum { TILE_IN = 0, TILE_TEST = 1, TILE_OUT = 2 };

struct PointList {                      // pts [N,3] (Decoders.forward, Mesher.eval_points)
    const float* pts;
    int64_t N;
    struct Tile { int64_t p0; int n; };
    __device__ int64_t ntiles() const { return (N + 63) / 64; }
    __device__ Tile tile(int64_t t) const { return Tile{t * 64, (int)min((int64_t)64, N - t * 64)}; }
    __device__ void point(const Tile& t, int j, float& x, float& y, float& z) const {
        const float* p = pts + (t.p0 + j) * 3;
        x = p[0]; y = p[1]; z = p[2];
    }
    __device__ int classify(const Tile&, const Bound&, int) const { return TILE_IN; }
    __device__ bool inside(const Tile&, float, float, float) const { return true; }
};

// The implicit grid (xs[ix], ys[iy], zs[iz]) of Mesher.get_grid_uniform, output [nx][ny][nz].  A tile is a run of at most
// 64 points of one z-row, i.e. a segment (the axes ascend).  Half-spaces (n, d): a point is inside when n.p + d <= 0 for
// all of them (an intersection, convex): a segment whose two ends are inside lies inside, one whose two ends are outside
// the same half-space lies outside.
struct GridPoints {
    const float* xs; const float* ys; const float* zs;
    int64_t nx, ny, nz, tpr;            // tpr: tiles per z-row
    const float4_t* hs;
    int nhs;
    struct Tile { int64_t p0; int n; int64_t ix, iy, z0; };
    __device__ int64_t ntiles() const { return nx * ny * tpr; }
    __device__ Tile tile(int64_t t) const {
        // the tile index is wave-uniform: say so, so that the tile's geometry and the half-space loads stay scalar
        t = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)t));
        const int64_t row = t / tpr, zt = t - row * tpr;
        Tile r;
        r.ix = row / ny;
        r.iy = row - r.ix * ny;
        r.z0 = zt * 64;
        r.p0 = row * nz + r.z0;
        r.n = (int)min((int64_t)64, nz - r.z0);
        return r;
    }
    __device__ void point(const Tile& t, int j, float& x, float& y, float& z) const {
        x = xs[t.ix]; y = ys[t.iy]; z = zs[t.z0 + j];
    }
    // the tile's class; each lane takes every 64th half-space, the wave votes
    __device__ int classify(const Tile& t, const Bound& bnd, int mask_outside) const {
        const float x = xs[t.ix], y = ys[t.iy], za = zs[t.z0], zb = zs[t.z0 + t.n - 1];
        if (mask_outside && !(x < bnd.hi[0] && x > bnd.lo[0] && y < bnd.hi[1] && y > bnd.lo[1] && zb > bnd.lo[2] &&
                              za < bnd.hi[2]))
            return TILE_OUT;
        bool both = false, one = false;
        for (int k = threadIdx.x & 63; k < nhs; k += 64) {
            bool oa, ob;
            ends_outside(hs[k], x, y, za, zb, oa, ob);
            both |= oa && ob;
            one |= oa || ob;
        }
        if (__any(both)) return TILE_OUT;
        return __any(one) ? TILE_TEST : TILE_IN;
    }
    __device__ static void ends_outside(const float4_t& h, float x, float y, float za, float zb, bool& oa, bool& ob) {
        const float base = h[0] * x + h[1] * y + h[3];
        oa = base + h[2] * za > 0.0f;
        ob = base + h[2] * zb > 0.0f;
    }
    // per point of a TILE_TEST tile: only the half-spaces that split the tile's segment can reject a point of it
    __device__ bool inside(const Tile& t, float x, float y, float z) const {
        const float za = zs[t.z0], zb = zs[t.z0 + t.n - 1];
        bool in = true;
        for (int k0 = 0; k0 < nhs; k0 += 64) {
            const int k = k0 + (threadIdx.x & 63);
            bool oa = false, ob = false;
            if (k < nhs) ends_outside(hs[k], x, y, za, zb, oa, ob);
            uint64_t split = __ballot(oa != ob);
            while (split) {
                const int j = __builtin_ctzll(split);
                split &= split - 1;
                const float4_t h = hs[k0 + j];
                if (h[0] * x + h[1] * y + h[3] + h[2] * z > 0.0f) in = false;
            }
        }
        return in;
    }
};

// LOWP: the mixed-precision tile (fp16 plane copies, bf16 MFMA decoders, as render_fwd_kernel's LOWP branches; channels-last
// only): saved features are the bf16 values the decoders consumed ([N,128] shorts, store_features_lp).
template <bool CL, bool SDF_ONLY, bool SAVE, typename Src, bool LOWP = false>
__global__ __launch_bounds__(256, LOWP ? DECODE_LP_WAVES : FWD_WAVES) void decode_fwd_kernel(const PlaneSet planes, const eslam_decoders_t dec,
                                                         const Bound bnd, const Src src,
                                                         float* __restrict__ raw, float* __restrict__ feat_out,
                                                         const int mask_outside) {
    static_assert(!LOWP || CL, "the half copies are channels-last");
    __shared__ __attribute__((aligned(16))) float wlds[2 * DEC_LDS];
    if (LOWP) stage_decoder_weights_lowp(wlds, dec, threadIdx.x, blockDim.x);
    else stage_decoder_weights(wlds, dec, threadIdx.x, blockDim.x);
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;                                  // MFMA role
    const int gp = gather_point<CL>(lane), gq = gather_piece<CL>(lane);     // gather role (LOWP: piece = channels 8gq..8gq+7)
    const int64_t ntiles = src.ntiles();

    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += (int64_t)gridDim.x * 4) {
        const typename Src::Tile tile = src.tile(t);
        const int64_t p0 = tile.p0;
        const int nvalid = tile.n;
        const int cls = src.classify(tile, bnd, mask_outside);
        if (cls == TILE_OUT) {          // (grid only) the whole tile is outside the bound or the half-spaces
            if (lane < nvalid) raw[p0 + lane] = -1.0f;
            continue;
        }
        const int nblk = (nvalid + 15) >> 4;
        float4_t out[2];
#pragma unroll
        for (int d = 0; d < (SDF_ONLY ? 1 : 2); ++d) {
            out[d] = LOWP ? *(const float4_t*)(lp_biases(wlds, d) + 32) : *(const float4_t*)(wlds + d * DEC_LDS + DEC_B3);
#pragma unroll 1
            for (int b = 0; b < nblk; ++b) {
                const int oz0 = opaque_zero(b);
                const int j = 16 * b + gp;
                const int64_t pb = p0 + j;
                float wx, wy, wz;
                src.point(tile, min(j, nvalid - 1), wx, wy, wz);
                const float px = norm_coord(wx, bnd.lo[0], bnd.hi[0]);
                const float py = norm_coord(wy, bnd.lo[1], bnd.hi[1]);
                const float pz = norm_coord(wz, bnd.lo[2], bnd.hi[2]);
                float feat[16];
                if (LOWP) {
                    gather_features_half(planes, d, px, py, pz, gq, feat, oz0);
                    if (SAVE) {
                        if (j < nvalid) store_features_lp(feat_out, pb, d, gq, feat);
                    }
                    to_mfma_role<true, 16>(feat, lane);
                    DecFragLP fl;
                    load_dec_frag_lp(fl, lp_weights(wlds, d) + oz0, lp_biases(wlds, d) + oz0, r, q);
                    float4_t a1, a2;
                    mlp_hidden_lp(fl, feat, a1, a2);
                    mlp_out_accum_lp(fl, a2, b, r, out[d]);
                    continue;
                }
                gather_features<CL>(planes, d, px, py, pz, gq, feat, oz0);
                if (SAVE) {
                    if (j < nvalid) store_features(feat_out, pb, d, gq, feat);
                }
                to_mfma_role<CL, 16>(feat, lane);
                DecFrag f;
                load_dec_frag(f, wlds + d * DEC_LDS + oz0, r, q);
                float4_t h1, h2;
                mlp_hidden(f, feat, h1, h2);
                mlp_out_accum(f, h2, b, r, out[d]);
            }
        }
        bool keep = true;
        if (cls == TILE_TEST) {         // (wave-uniform: every lane takes part in the half-space vote) Mesher.py:217
            float x, y, z;
            src.point(tile, min(lane, nvalid - 1), x, y, z);
            keep = src.inside(tile, x, y, z);
        }
        if (lane < nvalid) {
            float sdf = tanhf(out[0][0]);
            if (mask_outside) {     // Mesher.eval_points (Mesher.py:146-153): points not strictly inside the bound get -1
                float x, y, z;
                src.point(tile, lane, x, y, z);
                const bool in = x < bnd.hi[0] && x > bnd.lo[0] && y < bnd.hi[1] && y > bnd.lo[1] && z < bnd.hi[2] &&
                                z > bnd.lo[2];
                if (!in) sdf = -1.0f;
            }
            if (!keep) sdf = -1.0f;
            if (SDF_ONLY) {
                raw[p0 + lane] = sdf;
            } else {
                float4_t v;
                v[0] = sigmoidf_(out[1][0]);
                v[1] = sigmoidf_(out[1][1]);
                v[2] = sigmoidf_(out[1][2]);
                v[3] = sdf;
                *(float4_t*)(raw + (p0 + lane) * 4) = v;
            }
        }
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

static int render_fwd_common(const char* who, const eslam_plane_t* planes, const eslam_decoders_t* dec,
                             const float* bound6_host, const float* rays_o, const float* rays_d, const float* z_vals,
                             int R, int S, float* depth, float* rgb, float* sdf, float* raw_rgb, float* feat, float* hid,
                             const int32_t* ray_order, const LossIn* li, uint32_t* rng_bump, eslam_stream_t stream) {
    if (R <= 0) return 0;
    if (S <= 0 || S > ESLAM_MAX_SAMPLES) {
        eslam_set_error("%s: S=%d outside [1,%d]", who, S, ESLAM_MAX_SAMPLES);
        return 1;
    }
    if (!planes || !dec || !bound6_host || !rays_o || !rays_d || !z_vals || !depth || !rgb || !sdf) {
        eslam_set_error("%s: null argument", who);
        return 1;
    }
    if ((raw_rgb == nullptr) != (feat == nullptr)) {
        eslam_set_error("%s: raw_rgb and feat must both be given or both be NULL", who);
        return 1;
    }
    if (hid && !feat) {
        eslam_set_error("%s: the hidden layer is saved beside the features: feat is NULL", who);
        return 1;
    }
    if (hid && eslam_saved_hidden_floats(R, S) * 4 >= ((int64_t)1 << 32) - 256) {       // 32-bit byte offsets, as the features
        eslam_set_error("%s: %lld rays of %d samples exceed the 32-bit offset range of the saved hidden layer: split the batch", who,
                        (long long)R, S);
        return 1;
    }
    if (eslam_validate_planes(planes, 0, NPL)) return 1;
    PlaneSet ps;
    for (int i = 0; i < NPL; ++i) ps.p[i] = planes[i];
    const Bound bnd = make_bound(bound6_host);
    const bool cl = eslam_planes_channels_last(planes, 0, NPL);
    const bool save = feat != nullptr;
    if (save && (int64_t)R * S * 512 >= ((int64_t)1 << 32) - 256) {       // saved features are addressed with 32-bit byte offsets
        eslam_set_error("%s: %lld points exceed the 32-bit offset range of the saved-feature buffer (8.3 M): split the batch", who,
                        (long long)R * S);
        return 1;
    }
    const int nblocks = (R + 3) / 4;
    static const int resident = [] {        // workgroups the chip holds at once: FWD_WAVES waves per SIMD = FWD_WAVES workgroups per CU
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return ((FWD_WAVES * cus) / 8) * 8;
    }();
    // persistent only when the rays divide evenly over the resident workgroups (4096, 8192 rays ...): a static assignment of
    // 2.44 rays per wave (5000 rays) runs three rounds where the hardware's own dispatch of 1250 workgroups needs 2.5
    // (forward 95 -> 108 us at 5000 x 56)
    int nwg = ((nblocks + 7) / 8) * 8;
    if (nwg > resident && nwg % resident == 0) nwg = resident;
    dim3 grid(nwg), block(256);
    hipStream_t st = (hipStream_t)stream;
    const LossIn none = {};
    const int lowp = eslam_planes_lowp(planes);
    if (lowp < 0) return 1;
    float* hidp = lowp ? nullptr : hid;       // (the mixed-precision kernels save no hidden layer)
#define LAUNCH(CLv, SV, LS)                                                                                             \
    hipLaunchKernelGGL((render_fwd_kernel<CLv, SV, LS, false>), grid, block, 0, st, ps, *dec, bnd, rays_o, rays_d, z_vals, R, \
                       S, depth, rgb, sdf, raw_rgb, feat, hidp, (const int*)ray_order, LS ? *li : none, rng_bump)
#define LAUNCH_LP(SV, LS)                                                                                               \
    hipLaunchKernelGGL((render_fwd_kernel<true, SV, LS, true>), grid, block, 0, st, ps, *dec, bnd, rays_o, rays_d, z_vals, R, \
                       S, depth, rgb, sdf, raw_rgb, feat, hidp, (const int*)ray_order, LS ? *li : none, rng_bump)
    eslam_prof_begin(PROF_RENDER_FWD, st);
    if (lowp) {
        if (li) { if (save) LAUNCH_LP(true, true); else LAUNCH_LP(false, true); }
        else { if (save) LAUNCH_LP(true, false); else LAUNCH_LP(false, false); }
    } else if (li) {
        if (cl && save) LAUNCH(true, true, true);
        else if (cl) LAUNCH(true, false, true);
        else if (save) LAUNCH(false, true, true);
        else LAUNCH(false, false, true);
    } else {
        if (cl && save) LAUNCH(true, true, false);
        else if (cl) LAUNCH(true, false, false);
        else if (save) LAUNCH(false, true, false);
        else LAUNCH(false, false, false);
    }
#undef LAUNCH
#undef LAUNCH_LP
    eslam_prof_end(PROF_RENDER_FWD, st);
    return eslam_check_launch("render_fwd_kernel");
}

extern "C" int64_t eslam_saved_hidden_floats(int64_t R, int S) {
    if (R < 0 || S < 0) return -1;
    return 2 * R * (((int64_t)S + 15) >> 4) * 256;
}

extern "C" int eslam_render_fwd_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                  const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                  float* depth, float* rgb, float* sdf, float* raw_rgb, float* feat,
                                  const int32_t* ray_order, uint32_t* rng_bump, float* hidden, eslam_stream_t stream) {
    return render_fwd_common("eslam_render_fwd", planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, depth, rgb, sdf,
                             raw_rgb, feat, hidden, ray_order, nullptr, rng_bump, stream);
}

extern "C" int eslam_render_fwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                float* depth, float* rgb, float* sdf, float* raw_rgb, float* feat,
                                const int32_t* ray_order, uint32_t* rng_bump, eslam_stream_t stream) {
    return eslam_render_fwd_h(planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, depth, rgb, sdf, raw_rgb, feat, ray_order,
                              rng_bump, nullptr, stream);
}

extern "C" int eslam_render_fwd_loss_h(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                       const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                       float* depth, float* rgb, float* sdf, float* raw_rgb, float* feat,
                                       const int32_t* ray_order, const float* gt_depth, const float* gt_color,
                                       double truncation, const float* weights5_host, const uint8_t* ray_mask,
                                       float* scratch, float* acc, float* loss, uint32_t* rng_bump, float* hidden,
                                       eslam_stream_t stream) {
    if (!gt_depth || !gt_color || !weights5_host || !scratch || !acc) {
        eslam_set_error("eslam_render_fwd_loss: null loss argument");
        return 1;
    }
    if (R <= 0) {
        eslam_set_error("eslam_render_fwd_loss: empty batch");
        return 1;
    }
    LossIn li;
    li.gt_depth = gt_depth; li.gt_color = gt_color; li.ray_mask = ray_mask;
    li.scratch = scratch; li.acc = acc; li.loss = loss;
    li.det = eslam_deterministic();
    li.tr = make_trunc(truncation);
    li.w = LossW{weights5_host[0], weights5_host[1], weights5_host[2], weights5_host[3], weights5_host[4]};
    return render_fwd_common("eslam_render_fwd_loss", planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, depth, rgb,
                             sdf, raw_rgb, feat, hidden, ray_order, &li, rng_bump, stream);
}

extern "C" int eslam_render_fwd_loss(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                     const float* rays_o, const float* rays_d, const float* z_vals, int R, int S,
                                     float* depth, float* rgb, float* sdf, float* raw_rgb, float* feat,
                                     const int32_t* ray_order, const float* gt_depth, const float* gt_color,
                                     double truncation, const float* weights5_host, const uint8_t* ray_mask,
                                     float* scratch, float* acc, float* loss, uint32_t* rng_bump, eslam_stream_t stream) {
    return eslam_render_fwd_loss_h(planes, dec, bound6_host, rays_o, rays_d, z_vals, R, S, depth, rgb, sdf, raw_rgb, feat, ray_order,
                                   gt_depth, gt_color, truncation, weights5_host, ray_mask, scratch, acc, loss, rng_bump, nullptr,
                                   stream);
}

extern "C" int eslam_decode_fwd(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                                const float* pts, int64_t N, int flags, float* raw, float* feat,
                                eslam_stream_t stream) {
    if (N <= 0) return 0;
    if (flags & ~(ESLAM_DECODE_SDF_ONLY | ESLAM_DECODE_MASK_OUTSIDE)) {
        eslam_set_error("eslam_decode_fwd: unknown flags 0x%x", flags);
        return 1;
    }
    const int sdf_only = flags & ESLAM_DECODE_SDF_ONLY;
    const int mask_outside = (flags & ESLAM_DECODE_MASK_OUTSIDE) ? 1 : 0;
    if (!planes || !dec || !bound6_host || !pts || !raw) {
        eslam_set_error("eslam_decode_fwd: null argument");
        return 1;
    }
    if (sdf_only && feat) {
        eslam_set_error("eslam_decode_fwd: feat cannot be saved in sdf_only mode");
        return 1;
    }
    if (eslam_validate_planes(planes, 0, sdf_only ? 6 : NPL)) return 1;
    PlaneSet ps;
    for (int i = 0; i < NPL; ++i) ps.p[i] = planes[sdf_only && i >= 6 ? i - 6 : i];
    const Bound bnd = make_bound(bound6_host);
    const bool cl = eslam_planes_channels_last(planes, 0, sdf_only ? 6 : NPL);
    const int64_t ntiles = (N + 63) / 64;
    const int64_t nwg = (ntiles + 3) / 4;
    dim3 grid((unsigned)(nwg < 8192 ? nwg : 8192)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const PointList src{pts, N};
#define LAUNCH(CLv, SO, SV) \
    hipLaunchKernelGGL((decode_fwd_kernel<CLv, SO, SV, PointList>), grid, block, 0, st, ps, *dec, bnd, src, raw, feat, \
                       mask_outside)
#define LAUNCH_LP(SO, SV) \
    hipLaunchKernelGGL((decode_fwd_kernel<true, SO, SV, PointList, true>), grid, block, 0, st, ps, *dec, bnd, src, raw, feat, \
                       mask_outside)
    const int lowp = eslam_planes_lowp(ps.p);       // (the 12 descriptors the kernel reads: sdf_only repeats the geometry planes)
    if (lowp < 0) return 1;
    eslam_prof_begin(PROF_DECODE_FWD, st);
    if (lowp) {         // feat: [N,128] bf16
        if (sdf_only) LAUNCH_LP(true, false);
        else if (feat) LAUNCH_LP(false, true);
        else LAUNCH_LP(false, false);
    } else if (sdf_only) {
        if (cl) LAUNCH(true, true, false);
        else LAUNCH(false, true, false);
    } else if (feat) {
        if (cl) LAUNCH(true, false, true);
        else LAUNCH(false, false, true);
    } else {
        if (cl) LAUNCH(true, false, false);
        else LAUNCH(false, false, false);
    }
#undef LAUNCH
#undef LAUNCH_LP
    eslam_prof_end(PROF_DECODE_FWD, st);
    return eslam_check_launch("decode_fwd_kernel");
}

extern "C" int eslam_sdf_grid(const eslam_plane_t* planes, const eslam_decoders_t* dec, const float* bound6_host,
                              const float* xs, const float* ys, const float* zs, int64_t nx, int64_t ny, int64_t nz,
                              const float* halfspaces, int n_halfspaces, int flags, float* vol, eslam_stream_t stream) {
    if (flags & ~(ESLAM_DECODE_SDF_ONLY | ESLAM_DECODE_MASK_OUTSIDE)) {
        eslam_set_error("eslam_sdf_grid: unknown flags 0x%x", flags);
        return 1;
    }
    if (nx < 0 || ny < 0 || nz < 0 || n_halfspaces < 0) {
        eslam_set_error("eslam_sdf_grid: negative size");
        return 1;
    }
    if (nx == 0 || ny == 0 || nz == 0) return 0;
    if (!planes || !dec || !bound6_host || !xs || !ys || !zs || !vol || (n_halfspaces && !halfspaces)) {
        eslam_set_error("eslam_sdf_grid: null argument");
        return 1;
    }
    if ((uintptr_t)halfspaces % 16) {
        eslam_set_error("eslam_sdf_grid: halfspaces must be 16-byte aligned (float4)");
        return 1;
    }
    if (eslam_validate_planes(planes, 0, 6)) return 1;
    PlaneSet ps;
    for (int i = 0; i < NPL; ++i) ps.p[i] = planes[i >= 6 ? i - 6 : i];
    const Bound bnd = make_bound(bound6_host);
    const bool cl = eslam_planes_channels_last(planes, 0, 6);
    GridPoints src;
    src.xs = xs; src.ys = ys; src.zs = zs;
    src.nx = nx; src.ny = ny; src.nz = nz; src.tpr = (nz + 63) / 64;
    src.hs = (const float4_t*)halfspaces;
    src.nhs = n_halfspaces;
    const int64_t ntiles = nx * ny * src.tpr;
    const int64_t nwg = (ntiles + 3) / 4;
    dim3 grid((unsigned)(nwg < 8192 ? nwg : 8192)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int mask_outside = (flags & ESLAM_DECODE_MASK_OUTSIDE) ? 1 : 0;
    const int lowp = eslam_planes_lowp(ps.p);
    if (lowp < 0) return 1;
    if (lowp) hipLaunchKernelGGL((decode_fwd_kernel<true, true, false, GridPoints, true>), grid, block, 0, st, ps, *dec, bnd, src,
                                 vol, nullptr, mask_outside);
    else if (cl) hipLaunchKernelGGL((decode_fwd_kernel<true, true, false, GridPoints>), grid, block, 0, st, ps, *dec, bnd, src, vol,
                               nullptr, mask_outside);
    else hipLaunchKernelGGL((decode_fwd_kernel<false, true, false, GridPoints>), grid, block, 0, st, ps, *dec, bnd, src, vol,
                            nullptr, mask_outside);
    return eslam_check_launch("decode_fwd_kernel<grid>");
}
