// ba_sim.hip -- the BinaryAgreement state machine of many instances and nodes
// on the GPU, in the synchronous rounds of sim.hip: what a node emits in round
// t is delivered in round t + 1, and a node handles its inbox in (sender
// index, emission order).  Round 0 is propose(input) of every node that has
// an input.  One thread per (instance, node) runs the handlers of ba_node.hpp
// sequentially; a workgroup owns whole instances, and all threads of an
// instance walk the same inbox, sender by sender: the loop is uniform, the
// handlers diverge.
//
// The coin travels by reference (include/hbrbc.h): a Coin record names its
// sender's share of the epoch's coin slot, share_ok and coin hold what the G2
// kernels of pairing.hip computed for every share and slot.
//
// Adversaries transform what LEAVES a node (BaNode::emit); the node itself
// runs the honest handlers on what it receives and on its own messages.
//
// Kernel forms (hbrbc_ba_args.form): the state of an instance is a block of
// its nodes' cores -- epoch, flags, nine sender masks, as structures of arrays
// over the nodes, so a wave's access to one field is one coalesced request --
// followed by the nodes' future-epoch rings.  GLOBAL reads and writes the
// cores where they lie; STAGED copies the cores of the workgroup's instances
// into LDS for the round and back (the rings, touched only by messages of a
// future epoch and at an epoch change, stay in global memory): 1-2 % faster
// at N=64 and N=128 (tools/ba_bench.py), so GLOBAL is kept for
// the validator counts whose cores pass 64 KiB of LDS and as the plain form
// the staged ones are tested against.  STAGED runs at the compiler's register
// budget or at 3 waves/SIMD (_W3), GLOBAL at 3 waves.  Tried, not kept: the
// inbox counts and headers through scalar registers where a wave holds one
// instance (readfirstlane): 2.13 vs 2.08 ms at N=64, 6.85 vs 6.74 at N=128.
#include "launchers.hpp"

#include <hip/hip_runtime.h>

#include "ba_node.hpp"

namespace hbrbc {

namespace {

template <bool STAGED>
__device__ __forceinline__ void ba_round_body(const hbrbc_ba_args &a, int ipb) {
    extern __shared__ uint32_t ba_lds[];
    if (a.active && *a.active == 0u) return;   // quiescent (uniform: the whole block leaves)
    const int n = (int)a.n, Q = (int)a.queue_epochs;
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const size_t inst0 = (size_t)blockIdx.x * ipb;
    const int ni = (int)((a.count - inst0) < (size_t)ipb ? (a.count - inst0) : (size_t)ipb);
    const size_t cw = ba_core_words(n), ib = (size_t)n * ba_state_bytes(n, Q);
    const uint32_t icw = (uint32_t)(n * cw);   // core words of an instance
    if (STAGED) {
        for (uint32_t i = tid; i < (uint32_t)ni * icw; i += T) {
            const uint32_t li = i / icw;
            ba_lds[i] = reinterpret_cast<const uint32_t *>(a.state + (inst0 + li) * ib)[i - li * icw];
        }
        __syncthreads();
    }
    const int li = tid / n, local = tid - li * n;
    if (li < ni) {
        const size_t inst = inst0 + li;
        uint32_t nout = 0, bad = 0;
        ba_node_round(a, inst, local,
                      (STAGED ? ba_lds + (size_t)li * icw
                              : reinterpret_cast<uint32_t *>(a.state + inst * ib)) + local,
                      (size_t)n,
                      reinterpret_cast<uint16_t *>(a.state + inst * ib + 4 * (size_t)icw) +
                          (size_t)local * n * Q,
                      nout, bad);
        if (nout) atomicAdd(a.emitted, nout);
        if (bad) atomicOr(a.emitted + 1, bad);
    }
    if (STAGED) {
        __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)ni * icw; i += T) {
            const uint32_t li2 = i / icw;
            reinterpret_cast<uint32_t *>(a.state + (inst0 + li2) * ib)[i - li2 * icw] = ba_lds[i];
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void ba_round_kernel(hbrbc_ba_args a, int ipb) {
    ba_round_body<STAGED>(a, ipb);
}
// The same at 3 waves/SIMD (168 VGPRs and some spills instead of 230 at 2
// waves): N=128, whose workgroups are one instance of two waves, ran 6.74 ->
// 5.83 ms per tools/ba_bench.py run; N=64 (four instances a workgroup) 2.07
// -> 2.12 ms, and 4 waves/SIMD (128 VGPRs) lost at both (2.55, 6.31 ms).
template <bool STAGED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void
ba_round_w3_kernel(hbrbc_ba_args a, int ipb) {
    ba_round_body<STAGED>(a, ipb);
}

}  // namespace

hipError_t launch_ba_round(const hbrbc_ba_args &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const int n = (int)a.n;
    int ipb = n >= 128 ? 1 : 256 / n;
    if ((size_t)ipb > a.count) ipb = (int)a.count;
    const size_t per = 4 * (size_t)n * ba_core_words(n);   // LDS bytes per instance
    // AUTO: the LDS-staged form where an instance's cores fit 64 KiB (n <= 210
    // or so), at 3 waves/SIMD from n = 128 (see ba_round_w3_kernel); beyond,
    // the global form
    uint32_t form = a.form;
    if (form == HBRBC_BA_FORM_AUTO)
        form = per > 65536 ? (uint32_t)HBRBC_BA_FORM_GLOBAL
                           : (n >= 128 ? (uint32_t)HBRBC_BA_FORM_STAGED_W3
                                       : (uint32_t)HBRBC_BA_FORM_STAGED);
    const bool staged = form != HBRBC_BA_FORM_GLOBAL;
    const bool w3 = form != HBRBC_BA_FORM_STAGED;
    if (staged) {
        while (ipb > 1 && ipb * per > 65536) --ipb;
        if (ipb * per > 65536) return hipErrorInvalidValue;
    }
    const unsigned blocks = (unsigned)((a.count + ipb - 1) / ipb);
    const unsigned threads = (unsigned)(ipb * n);
    auto kern = staged ? (w3 ? ba_round_w3_kernel<true> : ba_round_kernel<true>)
                       : ba_round_w3_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), staged ? ipb * per : 0, s, a, ipb);
    return hipGetLastError();
}

}  // namespace hbrbc
