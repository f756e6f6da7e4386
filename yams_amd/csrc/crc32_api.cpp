// crc32_api.cpp — the batched CRC-32 behind the C ABI: header.uncompressedCRC32 of the compressed store
// (compressed_storage_engine.cpp:524) for every chunk of a batch, and the read side's check of it (:594-627,
// storage_engine.cpp:102-120), over device-resident bytes or host memory.
#include <cstring>
#include <vector>

#include "accel_ctx.h"
#include "crc32_host.h"
#include "crc32_launch.h"

using namespace yams_accel;

namespace {

constexpr uint64_t kMaxMessageBytes = 1ull << 40;

struct Pow2 { uint32_t v[crc32::kPow2]; };
const Pow2& pow2_table() {
    static const Pow2 t = [] {
        Pow2 p;
        p.v[0] = crc32::kOne >> 1;
        for (uint32_t k = 1; k < crc32::kPow2; ++k) p.v[k] = crc32::mulmod<crc32::kPolyCrc32>(p.v[k - 1], p.v[k - 1]);
        return p;
    }();
    return t;
}

// offsets / lengths are DEVICE arrays; results complete on return.
yams_status_t crc32_batch(yams_accel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                          uint32_t* out) {
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t* d_first; uint64_t* d_sums;
    YA_TRY(ws_get(ctx, "crc_seg_first", (n + 1) * 8, (void**)&d_first));
    YA_TRY(ws_get(ctx, "crc_block_sums", (crc_plan_blocks(n) + 1) * 8, (void**)&d_sums));
    {
        TimedRegion tr(ctx, "crc32_plan");
        YA_HIP(ctx, launch_crc32_plan(st, lengths, n, d_first, d_sums));
        tr.end();
    }
    // the one word read back: the number of segments sizes the workspace
    uint64_t* h_total;
    YA_TRY(pinned_get(ctx, 64, (void**)&h_total));
    YA_HIP(ctx, hipMemcpyAsync(h_total, d_first + n, 8, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    const uint64_t total = *h_total;
    // (lengths live on the device: what can be refused from the one word is a batch whose segments exceed n messages of 2^40 bytes)
    if (total > n * (kMaxMessageBytes / kCrcSegment)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a message longer than 2^40 bytes");
    uint32_t* d_pure;
    YA_TRY(ws_get(ctx, "crc_seg_pure", total * 4, (void**)&d_pure));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
    {
        TimedRegion tr(ctx, "crc32_segments");
        YA_HIP(ctx, launch_crc32_segments(st, data, offsets, lengths, d_first, n, total, static_cast<uint32_t>(cus), d_pure));
        tr.end();
    }
    {
        TimedRegion tr(ctx, "crc32_fold");
        YA_HIP(ctx, launch_crc32_fold(st, lengths, d_first, d_pure, n, out));
        tr.end();
    }
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

} // namespace

extern "C" {

uint32_t yams_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return crc32::combine<crc32::kPolyCrc32>(pow2_table().v, crc_a, crc_b, len_b);
}

yams_status_t yams_crc32_batch_device(yams_accel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lengths,
                                      uint64_t n_msgs, uint32_t* out_crc32) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (n_msgs == 0) return YAMS_OK;
    if (n_msgs >= (1ull << 31)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "more than 2^31 messages in one call");
    if (!offsets || !lengths || !out_crc32) return fail(ctx, YAMS_ERR_INVALID_ARG, "null message table");
    return crc32_batch(ctx, data, offsets, lengths, n_msgs, out_crc32);
}

yams_status_t yams_crc32_chunks_device(yams_accel_ctx* ctx, const uint8_t* data, const uint64_t* blob_offsets_host, uint64_t n_blobs,
                                       const yams_ingest_result_t* chunks, const uint8_t* select, uint32_t* out_crc32) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (!chunks) return fail(ctx, YAMS_ERR_INVALID_ARG, "null ingest result");
    const uint64_t n = chunks->n_chunks;
    if (n == 0) return YAMS_OK;
    if (n >= (1ull << 31) || n_blobs >= (1ull << 31)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "more than 2^31 messages in one call");
    if (!blob_offsets_host || n_blobs == 0 || !chunks->chunk_offset || !chunks->chunk_size || !chunks->chunk_blob || !out_crc32)
        return fail(ctx, YAMS_ERR_INVALID_ARG, "null chunk table");
    if (!data) return fail(ctx, YAMS_ERR_INVALID_ARG, "null data");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    uint64_t* d_blob_off; uint64_t* d_offs; uint64_t* d_lens;
    YA_TRY(ws_get(ctx, "crc_blob_off", n_blobs * 8, (void**)&d_blob_off));
    YA_TRY(ws_get(ctx, "crc_msg_off", n * 8, (void**)&d_offs));
    YA_TRY(ws_get(ctx, "crc_msg_len", n * 8, (void**)&d_lens));
    YA_HIP(ctx, hipMemcpyAsync(d_blob_off, blob_offsets_host, n_blobs * 8, hipMemcpyHostToDevice, st));
    YA_HIP(ctx, hipStreamSynchronize(st));      // (the caller's table may be pageable and is the caller's again on return)
    YA_HIP(ctx, launch_crc32_chunk_table(st, d_blob_off, chunks->chunk_blob, chunks->chunk_offset, chunks->chunk_size, select, n, d_offs, d_lens));
    return crc32_batch(ctx, data, d_offs, d_lens, n, out_crc32);
}

yams_status_t yams_crc32_verify_device(yams_accel_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lengths, uint64_t n,
                                       const uint32_t* expected_crc32, uint8_t* out_valid, uint64_t* out_n_invalid) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (out_n_invalid) *out_n_invalid = 0;
    if (n == 0) return YAMS_OK;
    if (!expected_crc32 || !out_valid) return fail(ctx, YAMS_ERR_INVALID_ARG, "null expected values / out_valid");
    (void)hipSetDevice(ctx->device);
    uint32_t* d_actual; unsigned long long* d_bad;
    YA_TRY(ws_get(ctx, "crc_verify_actual", n * 4, (void**)&d_actual));
    YA_TRY(ws_get(ctx, "crc_verify_count", 64, (void**)&d_bad));
    YA_TRY(yams_crc32_batch_device(ctx, data, offsets, lengths, n, d_actual));
    YA_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, ctx->stream));
    YA_HIP(ctx, launch_crc32_compare(ctx->stream, d_actual, expected_crc32, n, out_valid, d_bad));
    unsigned long long* h_bad;
    YA_TRY(pinned_get(ctx, 64, (void**)&h_bad));
    YA_HIP(ctx, hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    YA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out_n_invalid) *out_n_invalid = *h_bad;
    return YAMS_OK;
}

yams_status_t yams_crc32_many_host(yams_accel_ctx* ctx, const uint8_t* const* msgs_host, const size_t* lens, size_t n_msgs,
                                   uint32_t* out_crc32_host) {
    if (!ctx) return YAMS_ERR_INVALID_ARG;
    if (n_msgs == 0) return YAMS_OK;
    if (n_msgs >= (1ull << 31)) return fail(ctx, YAMS_ERR_UNSUPPORTED, "more than 2^31 messages in one call");
    if (!msgs_host || !lens || !out_crc32_host) return fail(ctx, YAMS_ERR_INVALID_ARG, "null message list");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> table(n_msgs * 2);
    uint64_t total = 0;
    for (size_t i = 0; i < n_msgs; ++i) {
        if (lens[i] && !msgs_host[i]) return fail(ctx, YAMS_ERR_INVALID_ARG, "null message");
        if (lens[i] > kMaxMessageBytes) return fail(ctx, YAMS_ERR_UNSUPPORTED, "a message longer than 2^40 bytes");
        table[i] = total; table[n_msgs + i] = lens[i];
        total += (lens[i] + 15) & ~static_cast<uint64_t>(15);  // every message starts on a granule of its own
    }
    uint8_t* d_data; uint64_t* d_table; uint32_t* d_crc;
    YA_TRY(ws_get(ctx, "crc_data", total + 64, (void**)&d_data));
    YA_TRY(ws_get(ctx, "crc_table", table.size() * 8, (void**)&d_table));
    YA_TRY(ws_get(ctx, "crc_out", n_msgs * 4, (void**)&d_crc));
    for (size_t i = 0; i < n_msgs; ++i)
        if (lens[i]) YA_HIP(ctx, hipMemcpyAsync(d_data + table[i], msgs_host[i], lens[i], hipMemcpyHostToDevice, st));
    YA_HIP(ctx, hipMemcpyAsync(d_table, table.data(), table.size() * 8, hipMemcpyHostToDevice, st));
    YA_TRY(crc32_batch(ctx, d_data, d_table, d_table + n_msgs, n_msgs, d_crc));
    YA_HIP(ctx, hipMemcpyAsync(out_crc32_host, d_crc, n_msgs * 4, hipMemcpyDeviceToHost, st));
    YA_HIP(ctx, hipStreamSynchronize(st));
    return YAMS_OK;
}

} // extern "C"
