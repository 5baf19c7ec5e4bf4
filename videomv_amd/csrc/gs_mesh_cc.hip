// gfx950 (MI355X) — connected components of a triangle mesh (videomv_amd/gs_mesh.py: mesh_components / drop_small_components; contract
// in include/vmv.h, "Connected components").  All integer: the result is a function of the SET of faces alone.
//   cc_init_kernel      one thread per vertex: parent[i] = i, face_count[i] = 0; thread 0 clears the status word
//   cc_hook_kernel      one thread per face: range test, then union (v0, v1) and (v0, v2)
//   cc_flatten_kernel   one thread per vertex: parent[i] = root(i).  No hook runs any more: the roots are final
//   cc_count_kernel     one thread per face: face_count[label[v0]] += 1, merged per wave and block before the atomicAdd (integer
//                       adds: any order and any grouping give the same sums)
// The parent array lives in ``label``.  A lock-free union-find: the LARGER root is always hooked under the SMALLER, with a compare-and-
// swap on the larger root's slot that succeeds only while it still is a root, and a path is shortened only by an atomicMin with the
// grandparent, so a slot that is not a root only ever moves to an ancestor and parent[i] <= i holds at every instant: no cycle can
// form, every chain strictly decreases, and the root that survives is the component's smallest index — the canonical label.  When
// the swap finds that the slot was no longer a root (another face hooked it first), the union goes on from the two roots as they are
// then.  Every parent read in a loop is an agent-scope atomic load (the L2s of the 8 XCDs are not coherent for plain loads, and a value
// kept in a register must not keep a loop alive); every parent write in the hook pass is an agent-scope atomic.
// Every loop spends from one per-thread budget of steps; a thread that runs out sets bit 1 of the status word and leaves, and a
// thread that starts after that leaves at once: a parent array that something else corrupted ends the kernel, it cannot hang it.
#include "gs_mesh_common.h"

namespace {

// A chain strictly decreases, so no walk of a sound parent array is longer than n_vertices, and a halving walk takes two links per
// step: the budget of a thread is 2 min(n_vertices, CC_MAX_STEPS) + CC_SLACK steps, four full-length walks and the retries of its two
// unions.  A walk also leaves at the first parent that is larger than its slot (or negative): the invariant itself is checked.
constexpr int CC_MAX_STEPS = 1 << 22, CC_SLACK = 4096;

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v's chain, halving the path on the way (parent[r] = min(parent[r], grandparent): still an ancestor, still <= r).
// -1: the budget ran out, or a slot held a parent above itself.
template <bool HALVE>
__device__ __forceinline__ int cc_root(int* parent, int v, int& budget) {
    int r = v;
    while (budget > 0) {
        --budget;
        const int p = cc_load(parent + r);
        if (p == r) return r;
        if ((unsigned)p > (unsigned)r) return -1;
        if (HALVE) {
            const int gp = cc_load(parent + p);
            if ((unsigned)gp > (unsigned)p) return -1;
            if (gp != p) cc_min(parent + r, gp);
            r = gp;
        } else {
            r = p;
        }
    }
    return -1;
}

// false: a walk gave up
__device__ __forceinline__ bool cc_union(int* parent, int a, int b, int& budget) {
    while (a != b) {
        a = cc_root<true>(parent, a, budget);
        b = cc_root<true>(parent, b, budget);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return true;                                               // hi was a root and hangs under lo now
        // hi had been hooked under seen < hi in the meantime: go on from there (both walks spend from the budget: the loop is bounded)
        a = seen;
        b = lo;
    }
    return true;
}

__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ label, int* __restrict__ face_count, int* __restrict__ status, const long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *status = 0;
    if (i >= n) return;
    label[i] = (int)i;
    face_count[i] = 0;
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const long* __restrict__ faces, const long stride, const long n_faces, const long n,
                                                      int* parent, int* status, const int steps) {
    long v[3];
    const int bad = mesh_load_face(faces, stride, n_faces, n, (long)blockIdx.x * 256 + threadIdx.x, v);
    if (bad > 0) atomicOr(status, MESH_STATUS_RANGE);
    if (bad || (cc_load(status) & MESH_STATUS_GAVE_UP)) return;
    int budget = steps;
    if (!(cc_union(parent, (int)v[0], (int)v[1], budget) && cc_union(parent, (int)v[0], (int)v[2], budget))) atomicOr(status, MESH_STATUS_GAVE_UP);
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, int* status, const long n, const int steps) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int budget = steps;
    // no halving here: the only write to a slot is its own final root, so a reader sees either the old parent or the root, both ancestors
    const int r = cc_root<false>(parent, (int)i, budget);
    if (r < 0) {
        atomicOr(status, MESH_STATUS_GAVE_UP);
        return;
    }
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void cc_count_kernel(const long* __restrict__ faces, const long stride, const long n_faces, const long n,
                                                       const int* __restrict__ label, int* __restrict__ face_count) {
    int r = -1;                                                        // this face's label; -1: nothing (left) to count
    long v[3];
    if (mesh_load_face(faces, stride, n_faces, n, (long)blockIdx.x * 256 + threadIdx.x, v) == 0) {
        r = label[v[0]];
        if (!mesh_in_range(r, n)) r = -1;                              // a label is in range unless the array was corrupted
    }
    // One add per face onto the label's slot is one contended address for a whole component (measured: 808 k faces, 775 k of them in
    // one component: 0.7-8.8 ms in this pass alone).  So the wave adds once per label it holds, and the label its first lane holds (in a
    // mesh, nearly always the label of all 64) is first merged over the block's four waves.  No thread leaves before the barrier.
    __shared__ int s_label[4], s_count[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long left = __ballot(r >= 0);
    int first_label = -1, first_count = 0;
    if (left) {
        first_label = __shfl(r, __ffsll(left) - 1);
        first_count = __popcll(__ballot(r == first_label));
        if (r == first_label) r = -1;
        left = __ballot(r >= 0);
    }
    if (lane == 0) {
        s_label[wave] = first_label;
        s_count[wave] = first_count;
    }
    for (int it = 0; it < 64 && left; ++it) {                          // every round retires at least one lane
        const int src = __ffsll(left) - 1, lab = __shfl(r, src);
        const unsigned long long same = __ballot(r == lab);
        if (lane == src) atomicAdd(face_count + lab, __popcll(same));
        if (r == lab) r = -1;
        left = __ballot(r >= 0);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_label[threadIdx.x] >= 0) {                // the lowest wave that holds a label adds for all that hold it
        const int lab = s_label[threadIdx.x];
        int total = 0;
        bool lowest = true;
        for (int w = 0; w < 4; ++w) {
            if (s_label[w] != lab) continue;
            total += s_count[w];
            lowest = lowest && w >= (int)threadIdx.x;
        }
        if (lowest) atomicAdd(face_count + lab, total);
    }
}

}  // namespace

extern "C" int vmv_gs_mesh_components(const VmvGsMeshComponentsParams* pp, void* stream) {
    if (!pp) return VMV_ENULL;
    const VmvGsMeshComponentsParams& p = *pp;
    if (!p.faces || !p.label || !p.face_count || !p.status) return VMV_ENULL;
    if (const int e = mesh_check_faces(p.faces, p.face_stride, p.n_faces, 0, p.n_vertices)) return e;
    if (((uintptr_t)p.label | (uintptr_t)p.face_count | (uintptr_t)p.status) & 3) return VMV_EALIGN;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long n = p.n_vertices, m = p.n_faces;
    const int steps = 2 * (int)(n < CC_MAX_STEPS ? n : CC_MAX_STEPS) + CC_SLACK;
    const dim3 vgrid((unsigned)((n + 255) / 256)), fgrid((unsigned)((m + 255) / 256));
    hipLaunchKernelGGL(cc_init_kernel, vgrid, dim3(256), 0, s, p.label, p.face_count, p.status, n);
    if (m > 0) {                                                       // no faces: identity labels, zero counts, no zero-sized launch
        hipLaunchKernelGGL(cc_hook_kernel, fgrid, dim3(256), 0, s, (const long*)p.faces, (long)p.face_stride, m, n, p.label, p.status, steps);
        hipLaunchKernelGGL(cc_flatten_kernel, vgrid, dim3(256), 0, s, p.label, p.status, n, steps);
        hipLaunchKernelGGL(cc_count_kernel, fgrid, dim3(256), 0, s, (const long*)p.faces, (long)p.face_stride, m, n, (const int*)p.label,
                           p.face_count);
    }
    return vmv_launch_status();
}
