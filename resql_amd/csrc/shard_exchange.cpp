// shard_exchange.cpp - the exchange layer of the rsq_multi_* paths (shard_exchange.h says what each piece is for).
#include "shard_exchange.h"

#include <thread>

#include "engine_internal.h"

namespace rsq {

ShardEvent::ShardEvent(const Context& ctx, bool timing) : device(ctx.device) {
    RSQ_HIP(hipSetDevice(device));
    RSQ_HIP(hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming));
}
ShardEvent::~ShardEvent() { if (ev) { (void)hipSetDevice(device); (void)hipEventDestroy(ev); } }
void ShardEvent::record(hipStream_t stream) const { RSQ_HIP(hipSetDevice(device)); RSQ_HIP(hipEventRecord(ev, stream)); }
double ShardEvent::msSince(const ShardEvent& from) const {
    float ms = 0;
    if (!ev || !from.ev) return 0;
    RSQ_HIP(hipSetDevice(device));
    return hipEventSynchronize(ev) == hipSuccess && hipEventElapsedTime(&ms, from.ev, ev) == hipSuccess ? (double)ms : 0;
}

void copyDeviceAsync(void* dst, int dstDevice, const void* src, int srcDevice, size_t bytes, hipStream_t stream) {
    if (dstDevice == srcDevice) RSQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    else RSQ_HIP(hipMemcpyPeerAsync(dst, dstDevice, src, srcDevice, bytes, stream));
}

int64_t gatherParts(Context& dst, void* base, const std::vector<GatherPart>& parts) {
    int64_t taken = 0;
    size_t at = 0;
    RSQ_HIP(hipSetDevice(dst.device));
    for (const GatherPart& p : parts) {
        if (!p.bytes) continue;
        if (p.ready) RSQ_HIP(hipStreamWaitEvent(dst.stream, p.ready, 0));
        copyDeviceAsync((char*)base + at, dst.device, p.ptr, p.src->device, p.bytes, dst.stream);
        if (p.src != &dst) taken += (int64_t)p.bytes;
        at += p.bytes;
    }
    return taken;
}

int64_t mergeDenseOnRoot(const std::vector<Query*>& shards, const std::vector<ShardEvent>& ready, int64_t* gathered, const char* disagree) {
    Context& root = shards[0]->ctx;
    int64_t nMin, nMax, nSum; void* out;
    queryDenseLayout(*shards[0], &nMin, &nMax, &nSum, &out);
    const int64_t words = nMin + nMax + nSum;
    std::vector<GatherPart> parts;
    for (size_t i = 0; i < shards.size(); i++) {
        int64_t a, b, c; void* part;
        queryDenseLayout(*shards[i], &a, &b, &c, &part);
        if (a != nMin || b != nMax || c != nSum) throw Error(RSQ_ERR_RUNTIME, disagree);
        parts.push_back({&shards[i]->ctx, part, (size_t)words * 8, ready[i].get()});
    }
    const int64_t taken = gatherParts(root, gathered, parts);
    mergePartialsAsync(root, gathered, (int)shards.size(), words, nMin, nMax, nSum, (int64_t*)out);
    return taken;
}

void enablePeerAccess(const std::vector<int>& devices, bool fromRootOnly) {
    for (size_t j = 0; j < (fromRootOnly ? 1 : devices.size()); j++)
        for (size_t i = 0; i < devices.size(); i++) {
            int can = 0;
            if (devices[i] == devices[j] || hipDeviceCanAccessPeer(&can, devices[j], devices[i]) != hipSuccess || !can) continue;
            RSQ_HIP(hipSetDevice(devices[j]));
            if (hipDeviceEnablePeerAccess(devices[i], 0) != hipSuccess) (void)hipGetLastError();
        }
}

void onShardThreads(int n, const std::function<void(int)>& step) {
    std::vector<std::string> errs((size_t)n);
    std::vector<int> status((size_t)n, RSQ_OK);
    std::vector<std::thread> th;
    for (int i = 0; i < n; i++)
        th.emplace_back([&, i] {
            try { step(i); }
            catch (const Error& e) { status[(size_t)i] = e.status; errs[(size_t)i] = e.what(); }
            catch (const std::exception& e) { status[(size_t)i] = RSQ_ERR_RUNTIME; errs[(size_t)i] = e.what(); }
        });
    for (auto& t : th) t.join();
    for (int i = 0; i < n; i++) if (status[(size_t)i] != RSQ_OK) throw Error(status[(size_t)i], "shard " + std::to_string(i) + ": " + errs[(size_t)i]);
}

}  // namespace rsq
