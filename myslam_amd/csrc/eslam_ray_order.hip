// Ray ordering as a launch of its own (eslam_ray_order, eslam_ray_order_clear): rays sorted by a key of their direction, so
// that neighbours in the order cross the same texels and the plane-gradient scatter (eslam_scatter.hip) can bundle them.
// The body is eslam_ray_order_dev.h, shared with step_front_kernel (eslam_sample.hip), which is what a training step runs.
#include "eslam_ray_order_dev.h"

// One launch, two independent roles chosen by the block number: blocks [0, n_order = chunks * ESLAM_RAY_ORDERS) order the rays
// (block b: chunk b / ESLAM_RAY_ORDERS, orientation b % ESLAM_RAY_ORDERS - the lowest numbers, so that they are placed first: they
// are the long ones), the blocks behind them zero clear_words floats at `clear` (16-byte aligned; the iteration's plane-gradient
// buffer) with 16-byte stores.  A replayed hipGraph pays ~3 us per node whatever its size (shard_prologue_kernel), and a memset
// node in front of the order held the order back by the memset's whole length.
__global__ __launch_bounds__(1024) void ray_order_kernel(const float* __restrict__ rays_o,
                                                         const float* __restrict__ rays_d, int R,
                                                         int* __restrict__ perm, int key_bits, const int n_order,
                                                         float* __restrict__ clear, const long long clear_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned hist[];       // ray_order_lds_bytes(key_bits): counters, then sorted ids
    if ((int)blockIdx.x >= n_order) {
        ray_clear_block(clear, clear_words, (int)blockIdx.x - n_order, (int)gridDim.x - n_order);
        return;
    }
    ray_order_block(rays_o, rays_d, R, perm, key_bits, (int)blockIdx.x, hist);
}

// the ordering workgroup's dynamic LDS is past the default limit: raised once per process
static int ray_order_allow_lds() {
    static bool done = false;
    if (done) return 0;
    if (hipFuncSetAttribute((const void*)ray_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            ORD_CELLS * (int)sizeof(unsigned)) != hipSuccess) {
        eslam_set_error("ray order: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
        return 2;
    }
    done = true;
    return 0;
}

// perm [R] <- rays ordered by direction; chunks of SORT_MAX rays are ordered independently.  clear / clear_bytes: a buffer the
// same launch zeroes (NULL / 0: none).
static int ray_order_launch(const char* who, const float* rays_o, const float* rays_d, int R, int32_t* perm, void* clear,
                            int64_t clear_bytes, eslam_stream_t stream) {
    if (ray_order_check_args(who, rays_o, rays_d, R, perm, clear, clear_bytes)) return 1;
    if (R <= 0 && clear_bytes == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = ray_order_allow_lds()) return rc;
    const int key_bits = ray_order_key_bits(R);
    const int n_clear = ray_clear_blocks(clear_bytes);
    const int n_order = ray_order_blocks(R);
    hipLaunchKernelGGL(ray_order_kernel, dim3(n_order + n_clear), dim3(1024), ray_order_lds_bytes(key_bits), st,
                       rays_o, rays_d, R, perm, key_bits, n_order, (float*)clear, (long long)(clear_bytes >> 2));
    return eslam_check_launch("ray_order_kernel");
}

extern "C" int eslam_ray_order(const float* rays_o, const float* rays_d, int R, int32_t* perm, eslam_stream_t stream) {
    if (R <= 0) return 0;
    return ray_order_launch("eslam_ray_order", rays_o, rays_d, R, perm, nullptr, 0, stream);
}

extern "C" int eslam_ray_order_clear(const float* rays_o, const float* rays_d, int R, int32_t* perm, void* clear_ptr,
                                     int64_t clear_bytes, eslam_stream_t stream) {
    return ray_order_launch("eslam_ray_order_clear", rays_o, rays_d, R, perm, clear_ptr, clear_bytes, stream);
}
