// shard_exchange.h - what the shards of one rsq_multi_* handle do to each other, each piece once: the event that orders one shard's stream
// behind another's, the gather of the shards' parts into one shard's memory, the dense group-by merge on the root, peer access, and the
// host threads the shards run on.  multi.cpp and engine_derived_multi.cpp are written on top of it.
#pragma once
#include "engine.h"

namespace rsq {

// An event that knows the device it was made on: made and destroyed with that device current.  Timing is kept for the pairs whose
// elapsed time is read; every other event is made with hipEventDisableTiming.
class ShardEvent {
  public:
    ShardEvent() = default;
    ShardEvent(const Context& ctx, bool timing);
    ShardEvent(ShardEvent&& o) noexcept : ev(o.ev), device(o.device) { o.ev = nullptr; }
    ShardEvent& operator=(ShardEvent&& o) noexcept { std::swap(ev, o.ev); std::swap(device, o.device); return *this; }
    ~ShardEvent();
    hipEvent_t get() const { return ev; }
    void record(hipStream_t stream) const;              // on a stream of its device
    double msSince(const ShardEvent& from) const;       // ms from `from` (same device) to this event, once this one has happened; 0 without them
  private:
    hipEvent_t ev = nullptr;
    int device = 0;
};

// `bytes` from device memory on srcDevice to device memory on dstDevice, enqueued on `stream` (dstDevice's): a device-to-device copy when
// both are one device, else a peer copy
void copyDeviceAsync(void* dst, int dstDevice, const void* src, int srcDevice, size_t bytes, hipStream_t stream);

// The shard-order gather.  A part: `bytes` at `ptr` on the shard whose context is `src`, complete once `ready` has happened (null: nothing
// to wait for).  The parts land back to back at `base`, in list order, copied on dst's stream, each behind its event; a part of 0 bytes
// is neither copied nor waited for.  Returns the bytes taken from other shards: a shard is its context, not its device ordinal.
struct GatherPart { const Context* src; const void* ptr; size_t bytes; hipEvent_t ready; };
int64_t gatherParts(Context& dst, void* base, const std::vector<GatherPart>& parts);

// The dense group-by merge on the root (shard 0): the shards' [min | max | sum] partial tables, which must agree on the layout (else
// `disagree` is thrown), gathered into `gathered` ([shards][words]) behind ready[i] (an empty handle: no wait) and merged into the
// root's own table by the engine's merge kernel.  Returns the bytes taken from other shards.
int64_t mergeDenseOnRoot(const std::vector<Query*>& shards, const std::vector<ShardEvent>& ready, int64_t* gathered, const char* disagree);

// peer copies between distinct GPUs go direct over xGMI where the pair allows it: every listed device (fromRootOnly: the first alone) is
// given access to every other one's memory
void enablePeerAccess(const std::vector<int>& devices, bool fromRootOnly);

// step(i) for every shard i < n, each on a host thread of its own (plans that need the host between kernels: join builds size their
// tables, hash aggregations grow theirs); the lowest failing shard's error is thrown as "shard i: ..."
void onShardThreads(int n, const std::function<void(int)>& step);

}  // namespace rsq
