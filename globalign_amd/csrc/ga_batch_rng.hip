// ga_batch_rng.hip -- batch_rng_kernel: the tie-break tables of a batch of alignments made where they are read
// (gfx950).  One wave per work item on a plain grid -- no ticket, no persistent loop, no wave waits
// for another; the only workgroup-wide step is building the quartet table in LDS.  The block-level pieces are
// ga_batch_rng.h's, shared with the CPU model (ga_batch_rng_selftest.cpp); here the lanes run them side by side,
// with a wave-scope fence wherever one lane reads what another wrote.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ga_batch_rng.h"
#include "ga_device.h"

namespace ga {

using namespace gabrng;

// One wave's memory operations to an address stay in order; the fence says so to the compiler and the memory model.
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(kLanes * kWavesPerGroup) batch_rng_kernel(RngArgs a) {
    __shared__ uint16_t quad_s[kQuadEntries];
    __shared__ uint32_t mt_s[kWavesPerGroup][kN];
    __shared__ uint32_t sym_s[kWavesPerGroup][kSymBytes / 4];
    __shared__ uint32_t acc_s[kWavesPerGroup][kAccBytes / 4];
#pragma clang loop vectorize(disable)
    for (int x = threadIdx.x; x < kQuadEntries; x += blockDim.x) quad_s[x] = quad_entry(x >> 8, x & 255);
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * kWavesPerGroup + w;
    if (t >= a.nitems) return;
    uint32_t* mt = mt_s[w];
    uint8_t* sym = reinterpret_cast<uint8_t*>(sym_s[w]);
    uint8_t* acc = reinterpret_cast<uint8_t*>(acc_s[w]);
    const Item it = a.items[t];
    const int steps = __builtin_amdgcn_readfirstlane(it.steps);
    const int blocks = __builtin_amdgcn_readfirstlane((int)max_blocks(steps, a.cap_words_per_dispatch));
    uint32_t* tab = a.tab + it.tab_off;

    // random.seed(seed): init_by_array on the shared base array, one lane (about 1250 dependent steps, once per item)
    for (int k = lane; k < kN; k += kLanes) mt[k] = a.base[k];
    wave_fence();
    if (lane == 0) seed_array(mt, it.seed);
    wave_fence();

    int done = 0;          // dispatches whose entries are stored
    uint32_t carry = 0;    // accepted draws of the unfinished dispatch, at acc[0 .. carry)
    for (int b = 0; b < blocks && done < steps; b++) {
        for (int c = 0; c < kTwistChunks; c++) {
            const uint32_t v = twist_read(mt, c, lane);
            wave_fence();
            twist_write(mt, c, lane, v);
            wave_fence();
        }
        uint32_t B[kPasses], mine[kPasses];
#pragma unroll
        for (int p = 0; p < kPasses; p++) B[p] = symbols_lane(mt, p, lane, sym);
        wave_fence();
        // (the same in every lane: said to the compiler, so that the block loop stays a scalar branch)
        const uint32_t total = __builtin_amdgcn_readfirstlane(run_automaton(quad_s, sym, carry, lane, mine));
#pragma unroll
        for (int p = 0; p < kPasses; p++) scatter_lane(quad_s, B[p], mine[p], p, lane, acc);
        wave_fence();
        entries_lane(acc, total, lane, done, steps, tab);
        const uint8_t v = carry_read(acc, total, lane);
        wave_fence();
        carry_write(acc, total, lane, v);
        wave_fence();
        done += (int)(total / kDraws);
        carry = total % kDraws;
    }
    if (lane == 0) a.status[t] = done >= steps ? kComplete : kCapReached;
}

// one wave per item; returns the workgroups launched
int launch_batch_rng(hipStream_t s, const RngArgs& a) {
    const int groups = (int)((a.nitems + kWavesPerGroup - 1) / kWavesPerGroup);
    if (groups > 0) batch_rng_kernel<<<groups, kLanes * kWavesPerGroup, 0, s>>>(a);
    return groups;
}

}  // namespace ga
