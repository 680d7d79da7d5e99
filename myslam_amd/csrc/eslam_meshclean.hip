// Mesh clean-up: the graph work behind src/tools/clean_mesh.py (trimesh's merge_vertices / process() and the
// connected-component filter of NICE-SLAM's remove_small_geometry, without trimesh or scipy).
//
//   weld        rep[v] = the smallest index whose position equals v's.  An open-addressing table of vertex indices
//               (capacity a power of two >= 2 V, cleared to -1): a vertex claims the first empty slot of its probe
//               sequence with atomicCAS(-1 -> v), or meets a slot that holds a vertex at its own position and lowers
//               it with atomicMin.  A slot goes from empty to one position for good, and only indices of that position
//               are ever written to it, so every vertex of a position ends in the same slot whatever the order.  A
//               second launch looks the slot's final value up.
//   components  label[v] = the smallest index of v's component (faces joined through shared vertices).  Lock-free
//               union-find in `label` itself: parent[x] <= x always; a union finds both roots and hangs the larger
//               under the smaller with atomicMin, and when the value handed back shows that the larger was no root
//               any more it goes on with the pair (handed-back parent, smaller root).  A second launch flattens.
//   sizes       face_count[label of the face's first corner] += 1, aggregated in the wave before the atomic.
//
// Rules kept by all three: no thread waits for another's progress (no flag, no lock); every loop
// is bounded by a strictly falling index or by the table's capacity; words that other workgroups update during the
// launch are read with relaxed agent-scope atomic loads (a CU's L1 is never refreshed by other CUs' stores), and a stale
// value is still harmless: an older table entry has the same position, an older parent joins the same component, and
// every decision is taken on what a returning atomic hands back.  Launch-to-launch visibility is the kernel boundary.
#include "eslam_common.h"

#define MCL_THREADS 256
#define MCL_MAX_BLOCKS (1 << 16)                    // grid-stride loops beyond this many workgroups
#define MCL_WAVE_ROUNDS 4                           // labels a wave aggregates before its lanes add on their own

static int mcl_blocks(int64_t n) {
    const int64_t b = (n + MCL_THREADS - 1) / MCL_THREADS;
    return (int)(b < 1 ? 1 : b > MCL_MAX_BLOCKS ? MCL_MAX_BLOCKS : b);
}

__device__ __forceinline__ int32_t mcl_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void mcl_store(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------
// weld
// ---------------------------------------------------------------------------------------------------------
struct WeldKey {
    uint32_t x, y, z;
    bool finite;
};

// a coordinate's bits with -0 turned into +0 (integer work only: denormals stay what they are)
__device__ __forceinline__ uint32_t weld_bits(float f) {
    const uint32_t b = __float_as_uint(f);
    return b == 0x80000000u ? 0u : b;
}

__device__ __forceinline__ WeldKey weld_key(const float* __restrict__ verts, int64_t v) {
    WeldKey k;
    k.x = weld_bits(verts[3 * v]);
    k.y = weld_bits(verts[3 * v + 1]);
    k.z = weld_bits(verts[3 * v + 2]);
    // NaN or infinity: all exponent bits set
    k.finite = (k.x & 0x7f800000u) != 0x7f800000u && (k.y & 0x7f800000u) != 0x7f800000u &&
               (k.z & 0x7f800000u) != 0x7f800000u;
    return k;
}

__device__ __forceinline__ bool weld_same(const WeldKey& a, const WeldKey& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

__device__ __forceinline__ uint32_t weld_hash(const WeldKey& k) {
    uint32_t h = k.x * 0x9e3779b1u ^ (k.y * 0x85ebca77u + 0x165667b1u) ^ (k.z * 0xc2b2ae3du + 0x27d4eb2fu);
    h ^= h >> 16;                                   // murmur3's finaliser
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// One vertex per lane.  At most `cap` probes; the table has cap >= 2 V slots, so an empty one always turns up.
__global__ __launch_bounds__(MCL_THREADS) void weld_insert_kernel(const float* __restrict__ verts, int64_t V,
                                                                  int32_t* __restrict__ table, uint32_t cap) {
    const uint32_t mask = cap - 1;
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * MCL_THREADS + threadIdx.x; v < V; v += stride) {
        const WeldKey k = weld_key(verts, v);
        if (!k.finite) continue;
        uint32_t slot = weld_hash(k) & mask;
        for (uint32_t n = 0; n < cap; ++n, slot = (slot + 1) & mask) {
            int32_t cur = mcl_load(table + slot);
            if (cur < 0) {
                cur = atomicCAS(table + slot, -1, (int32_t)v);
                if (cur < 0) break;                                 // the slot is this position's now
            }
            // cur: a vertex this slot holds or held; the slot's position never changes
            if (weld_same(k, weld_key(verts, cur))) {
                if (cur > v) atomicMin(table + slot, (int32_t)v);   // (a newer value is lower still: nothing to do then either)
                break;
            }
        }
    }
}

// after the insert launch the table is final: plain loads
__global__ __launch_bounds__(MCL_THREADS) void weld_lookup_kernel(const float* __restrict__ verts, int64_t V,
                                                                  const int32_t* __restrict__ table, uint32_t cap,
                                                                  int32_t* __restrict__ rep) {
    const uint32_t mask = cap - 1;
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * MCL_THREADS + threadIdx.x; v < V; v += stride) {
        const WeldKey k = weld_key(verts, v);
        int32_t r = -1;
        if (k.finite) {
            uint32_t slot = weld_hash(k) & mask;
            for (uint32_t n = 0; n < cap; ++n, slot = (slot + 1) & mask) {
                const int32_t cur = table[slot];
                if (cur < 0) break;                                 // (cannot happen: v was inserted)
                if (weld_same(k, weld_key(verts, cur))) {
                    r = cur;
                    break;
                }
            }
        }
        rep[v] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------
// components
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MCL_THREADS) void cc_init_kernel(int32_t* __restrict__ parent, int64_t V) {
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * MCL_THREADS + threadIdx.x; v < V; v += stride) parent[v] = (int32_t)v;
}

// The root above x as far as this thread can see it: parent[.] <= . and the walk strictly falls until it meets a word
// that holds its own index.  On the way x is re-hung under its grandparent (path halving): an atomicMin, so the word
// only falls and stays an ancestor.  A stale read is an older ancestor or an older member of the same component.
__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = mcl_load(parent + x);
        if (p >= x) return x;                                       // (p == x: a root; p > x cannot happen)
        const int32_t g = mcl_load(parent + p);
        if (g < p) atomicMin(parent + x, g);
        x = g < p ? g : p;
    }
}

__device__ __forceinline__ void cc_union(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        if (ra > rb) {
            const int32_t t = ra;
            ra = rb;
            rb = t;
        }
        const int32_t old = atomicMin(parent + rb, ra);             // the decision: what the atomic hands back
        if (old == rb) break;                                       // rb was a root and now hangs under ra
        // rb had the parent `old` < rb already; it now hangs under min(old, ra), and old and ra remain to be joined.
        // Both are below rb: the larger of the pair strictly falls, so the loop ends.
        rb = cc_find(parent, old);
        ra = cc_find(parent, ra);
    }
}

__global__ __launch_bounds__(MCL_THREADS) void cc_union_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                               int32_t* __restrict__ parent) {
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t f = (int64_t)blockIdx.x * MCL_THREADS + threadIdx.x; f < F; f += stride) {
        const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a != b) cc_union(parent, a, b);
        if (b != c) cc_union(parent, b, c);
    }
}

// label[v] = the root above v.  Roots no longer change in this launch; the words on the way are overwritten by other
// lanes with that same root, so whichever value a load returns, the walk ends at it.
__global__ __launch_bounds__(MCL_THREADS) void cc_flatten_kernel(int32_t* __restrict__ label, int64_t V) {
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * MCL_THREADS + threadIdx.x; v < V; v += stride) {
        int32_t x = (int32_t)v;
        for (;;) {
            const int32_t p = mcl_load(label + x);
            if (p >= x) break;
            x = p;
        }
        if (x != (int32_t)v) mcl_store(label + v, x);
    }
}

// ---------------------------------------------------------------------------------------------------------
// component sizes
// ---------------------------------------------------------------------------------------------------------
// One face per lane, the loop uniform over the workgroup.  Up to MCL_WAVE_ROUNDS times the lanes that share the first
// pending lane's label leave together with one add of their number; whoever is left adds 1 on its own.
__global__ __launch_bounds__(MCL_THREADS) void cc_sizes_kernel(const int32_t* __restrict__ faces, int64_t F,
                                                               const int32_t* __restrict__ label,
                                                               int32_t* __restrict__ face_count) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t stride = (int64_t)gridDim.x * MCL_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * MCL_THREADS; base < F; base += stride) {
        const int64_t f = base + threadIdx.x;
        bool todo = f < F;
        const int32_t l = todo ? label[faces[3 * f]] : 0;
        for (int r = 0; r < MCL_WAVE_ROUNDS; ++r) {
            const unsigned long long pending = __ballot(todo);
            if (!pending) break;
            const int leader = __ffsll(pending) - 1;
            const int32_t L = __shfl(l, leader, WAVE);
            const bool same = todo && l == L;
            const unsigned long long m = __ballot(same);
            if (lane == leader) atomicAdd(face_count + L, __popcll(m));
            todo = todo && !same;
        }
        if (todo) atomicAdd(face_count + l, 1);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool mcl_count_ok(const char* who, const char* what, int64_t n) {
    if (n < 0 || n > ESLAM_MESH_MAX_COUNT) {
        eslam_set_error("%s: %lld %s (0 .. 2^30)", who, (long long)n, what);
        return false;
    }
    return true;
}

// slots of the weld table: the power of two >= 2 V, at least ESLAM_MESH_WELD_MIN_SLOTS
static int64_t weld_slots(int64_t n_verts) {
    int64_t cap = ESLAM_MESH_WELD_MIN_SLOTS;
    while (cap < 2 * n_verts) cap <<= 1;
    return cap;
}

extern "C" int64_t eslam_mesh_weld_workspace_bytes(int64_t n_verts) {
    if (!mcl_count_ok("eslam_mesh_weld_workspace_bytes", "vertices", n_verts)) return -1;
    return 4 * weld_slots(n_verts);
}

extern "C" int eslam_mesh_weld(const float* verts, int64_t n_verts, void* workspace, int32_t* rep, eslam_stream_t stream) {
    if (!mcl_count_ok("eslam_mesh_weld", "vertices", n_verts)) return 1;
    if (n_verts == 0) return 0;
    if (!verts || !workspace || !rep) {
        eslam_set_error("eslam_mesh_weld: null argument");
        return 1;
    }
    const int64_t cap = weld_slots(n_verts);
    hipStream_t st = (hipStream_t)stream;
    int32_t* table = (int32_t*)workspace;
    if (hipMemsetAsync(table, 0xff, (size_t)cap * 4, st) != hipSuccess) {
        eslam_set_error("eslam_mesh_weld: memset failed");
        return 2;
    }
    hipLaunchKernelGGL(weld_insert_kernel, dim3(mcl_blocks(n_verts)), dim3(MCL_THREADS), 0, st, verts, n_verts, table,
                       (uint32_t)cap);
    if (eslam_check_launch("weld_insert_kernel")) return 1;
    hipLaunchKernelGGL(weld_lookup_kernel, dim3(mcl_blocks(n_verts)), dim3(MCL_THREADS), 0, st, verts, n_verts, table,
                       (uint32_t)cap, rep);
    return eslam_check_launch("weld_lookup_kernel");
}

extern "C" int eslam_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t* label,
                                     eslam_stream_t stream) {
    if (!mcl_count_ok("eslam_mesh_components", "faces", n_faces) || !mcl_count_ok("eslam_mesh_components", "vertices", n_verts))
        return 1;
    if (n_verts == 0) {
        if (n_faces > 0) {
            eslam_set_error("eslam_mesh_components: %lld faces over no vertices", (long long)n_faces);
            return 1;
        }
        return 0;
    }
    if (!label || (n_faces > 0 && !faces)) {
        eslam_set_error("eslam_mesh_components: null argument");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_init_kernel, dim3(mcl_blocks(n_verts)), dim3(MCL_THREADS), 0, st, label, n_verts);
    if (eslam_check_launch("cc_init_kernel")) return 1;
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(cc_union_kernel, dim3(mcl_blocks(n_faces)), dim3(MCL_THREADS), 0, st, faces, n_faces, label);
    if (eslam_check_launch("cc_union_kernel")) return 1;
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(mcl_blocks(n_verts)), dim3(MCL_THREADS), 0, st, label, n_verts);
    return eslam_check_launch("cc_flatten_kernel");
}

extern "C" int eslam_mesh_component_sizes(const int32_t* faces, int64_t n_faces, const int32_t* label, int64_t n_verts,
                                          int32_t* face_count, eslam_stream_t stream) {
    if (!mcl_count_ok("eslam_mesh_component_sizes", "faces", n_faces) ||
        !mcl_count_ok("eslam_mesh_component_sizes", "vertices", n_verts))
        return 1;
    if (n_verts == 0) {
        if (n_faces > 0) {
            eslam_set_error("eslam_mesh_component_sizes: %lld faces over no vertices", (long long)n_faces);
            return 1;
        }
        return 0;
    }
    if (!face_count || (n_faces > 0 && (!faces || !label))) {
        eslam_set_error("eslam_mesh_component_sizes: null argument");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(face_count, 0, (size_t)n_verts * 4, st) != hipSuccess) {
        eslam_set_error("eslam_mesh_component_sizes: memset failed");
        return 2;
    }
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(mcl_blocks(n_faces)), dim3(MCL_THREADS), 0, st, faces, n_faces, label, face_count);
    return eslam_check_launch("cc_sizes_kernel");
}
