// host_stage.h — the staging of one _host call: the one rule by which a _host twin brings its host arrays to the device, makes
// room for its outputs and brings them back.  A twin reads: its checks -> its up / room lines -> YA_TRY(hs.status()) -> the
// _device twin -> its down lines -> return hs.finish().
//
//  - Sticky status.  After the first failure (ws_get refused, a copy failed) up and room return nullptr, down does nothing and
//    nothing more is enqueued.  The failure is on the context already (fail / hip_fail) and carries their status code:
//    YAMS_ERR_RESOURCE_EXHAUSTED from ws_get, hip_fail's mapping for a copy.
//  - Every buffer is 16 bytes longer than asked, so count == 0 still has an address and a kernel's vector tail has room.
//  - Slot names are the callers': the entries of a family share their buffers by name.
//  - down is only ever called after the _device twin returned YAMS_OK.  That is the whole of "a refusal writes nothing": the
//    twin's own checks come before HostStage exists, status() before the _device call, and nothing else writes host memory.
//
// up enqueues its copy at once, so a later slot may grow while an earlier upload is in flight.  That is safe: every slot is a
// device allocation of its own (ws_get frees and replaces only the slot it was asked for, and synchronises the stream before
// it frees), so growing slot B neither moves nor frees slot A.
#pragma once
#include "accel_ctx.h"

namespace yams_accel {

class HostStage {
public:
    explicit HostStage(yams_accel_ctx* ctx) : ctx_(ctx) { (void)hipSetDevice(ctx->device); }
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;

    // Device room for count elements (an address for count == 0 too).
    template <class T> T* room(const char* slot, size_t count) {
        void* p = nullptr;
        if (st_ == YAMS_OK) st_ = ws_get(ctx_, slot, count * sizeof(T) + 16, &p);
        return st_ == YAMS_OK ? static_cast<T*>(p) : nullptr;
    }
    // A device copy of host[0 .. count): a null host pointer stays null; count == 0 gives an address and copies nothing.
    template <class T> const T* up(const char* slot, const T* host, size_t count) {
        if (!host) return nullptr;
        T* d = room<T>(slot, count);
        if (d && count) hip(staged_h2d(d, host, count * sizeof(T), ctx_->stream), "host stage upload");
        return st_ == YAMS_OK ? d : nullptr;
    }
    // Enqueue device -> host of count elements; nothing for count == 0 or a null host pointer.
    template <class T> void down(T* host, const T* dev, size_t count) {
        if (st_ == YAMS_OK && host && count)
            hip(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx_->stream), "host stage download");
    }
    yams_status_t status() const { return st_; }      // the first failure; sticky
    // One hipStreamSynchronize, then status(); may be called once per slice, and before a host temporary that was uploaded dies.
    yams_status_t finish() {
        if (st_ == YAMS_OK) hip(hipStreamSynchronize(ctx_->stream), "host stage synchronise");
        return st_;
    }

private:
    void hip(hipError_t e, const char* what) { if (e != hipSuccess) st_ = hip_fail(ctx_, e, what); }
    yams_accel_ctx* ctx_;
    yams_status_t st_ = YAMS_OK;
};

} // namespace yams_accel
