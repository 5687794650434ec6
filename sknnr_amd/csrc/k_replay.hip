// k_replay.hip -- kernel translation unit: stored neighbour tiles into the pipeline's full-layout tile (replay.hip.h) behind launch.hip.h.
#define SKNNR_KERNELS_REPLAY 1  // this unit defines the kernels of replay.hip.h
#include "launch.hip.h"

namespace sknnr {
namespace launch {

long replay_blocks(long n) { return (n + kReplayWgPixels - 1) / kReplayWgPixels; }

namespace {
template <typename I, typename D>
hipError_t replay_layout(const ReplayArgs& a, bool planes, unsigned blocks, hipStream_t st) {
    if (planes) replay_kernel<I, D, true><<<dim3(blocks), dim3(kReplayThreads), 0, st>>>(a);
    else replay_kernel<I, D, false><<<dim3(blocks), dim3(kReplayThreads), 0, st>>>(a);
    return hipGetLastError();
}
template <typename I>
hipError_t replay_dist(const ReplayArgs& a, int dist_kind, bool planes, unsigned blocks, hipStream_t st) {
    switch (dist_kind) {
        case kReplayDistNone: return replay_layout<I, ReplayNoDist>(a, planes, blocks, st);
        case kReplayDistF32: return replay_layout<I, float>(a, planes, blocks, st);
        case kReplayDistF64: return replay_layout<I, double>(a, planes, blocks, st);
    }
    return hipErrorInvalidValue;
}
}  // namespace

hipError_t replay(const ReplayArgs& a, int idx_bytes, int dist_kind, bool planes, hipStream_t st) {
    if (a.n < 0 || a.k < 1 || a.k > a.ks || a.n_ref < 1) return hipErrorInvalidValue;
    if (idx_bytes != 4 && idx_bytes != 8) return hipErrorInvalidValue;
    if (dist_kind < kReplayDistNone || dist_kind > kReplayDistF64) return hipErrorInvalidValue;
    if (!a.rec || (a.n > 0 && (!a.idx || !a.out_idx || !a.bad))) return hipErrorInvalidValue;
    if (dist_kind != kReplayDistNone && a.n > 0 && (!a.dist || !a.out_dist)) return hipErrorInvalidValue;
    if (a.id_sorted && (!a.id_perm || a.m < 1 || a.m > 0x7fffffffL)) return hipErrorInvalidValue;
    if (planes && a.in_stride < a.n) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = replay_blocks(a.n);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    return idx_bytes == 4 ? replay_dist<int32_t>(a, dist_kind, planes, (unsigned)blocks, st)
                          : replay_dist<long>(a, dist_kind, planes, (unsigned)blocks, st);
}

hipError_t replay_blank(const ReplayBlankArgs& a, hipStream_t st) {
    if (a.n < 0 || a.k < 1 || (a.n > 0 && (!a.bad || !a.idx)) || (a.pred && a.pred_cols < 1)) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const long blocks = (a.n + kReplayThreads - 1) / kReplayThreads;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    replay_blank_kernel<<<dim3((unsigned)blocks), dim3(kReplayThreads), 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace sknnr
