// crc32_kernels.hip — batched CRC-32 on the device: the uncompressedCRC32 of CompressedStorageEngine's
// headers (compressed_storage_engine.cpp:49-59, 524) and the read side's check of it (storage_engine.cpp:102-120,
// compression_utils.cpp:31-52) for many messages per call.
//
// CRC is linear over GF(2), so the unit of work is a SEGMENT of kCrcSegment bytes, not a message:
//   plan      segment counts per message -> exclusive prefix sum (segment s belongs to message i iff
//             seg_first[i] <= s < seg_first[i + 1]); an empty message owns one empty segment
//   segments  one wave per segment, a wave takes a contiguous run of segments whatever messages they belong to: one
//             64 MiB message beside 20 000 tiny ones is 16 384 + 20 000 equal units.  The wave reads 64 adjacent
//             16-byte granules per step (1 KiB contiguous); lane l keeps a register over granules l, l + 64, ...
//             (reg = reg * x^8192 ^ pure(granule): the stride operator), brings it to the segment's end with ONE
//             multiplication by x^(8 m), m < 1024 (a per-lane constant), and the wave xor-reduces.
//   fold      one wave per message: lanes Horner over contiguous runs of the message's full segments with the fixed
//             x^(8 S) operator, one arbitrary-length shift each (square-and-multiply over x^(2^k)), xor-reduce, final xor.
// The polynomial is a template parameter; only the standard CRC-32 is instantiated (nothing else has an oracle).
#include "crc32_host.h"
#include "crc32_launch.h"

namespace yams_accel {

namespace {

constexpr uint32_t kPoly = crc32::kPolyCrc32;
using CrcTables = crc32::Tables<kCrcSegment>;

constexpr CrcTables build_tables() {
    CrcTables t{};
    crc32::make_tables<kPoly, kCrcSegment>(t);
    return t;
}
__device__ const CrcTables g_crc_tables = build_tables();

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), m, 64));
    return v;
}

// Exclusive scan of one value per thread over a workgroup of 256; `total` receives the sum.  buf: 256 words of LDS.
__device__ __forceinline__ uint64_t block_scan_256(uint64_t v, uint64_t* buf, uint64_t* total) {
    const uint32_t t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    uint64_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t other = t >= d ? buf[t - d] : 0;
        __syncthreads();
        inc += other;
        buf[t] = inc;
        __syncthreads();
    }
    *total = buf[255];
    __syncthreads();
    return inc - v;
}

} // namespace

__global__ __launch_bounds__(256) void crc32_chunk_table_kernel(const uint64_t* blob_off, const uint32_t* chunk_blob,
                                                                const uint64_t* chunk_offset, const uint64_t* chunk_size,
                                                                const uint8_t* select, uint64_t n, uint64_t* offs, uint64_t* lens) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    offs[i] = blob_off[chunk_blob[i]] + chunk_offset[i];
    lens[i] = (select && !select[i]) ? 0 : chunk_size[i];
}

// ---- plan ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crc32_plan_count_kernel(const uint64_t* lens, uint64_t n_msgs, uint64_t* seg_first,
                                                               uint64_t* block_sums) {
    __shared__ uint64_t buf[256];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kCrcPlanItems + threadIdx.x * 4ull;
    uint64_t c[4], mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c[q] = base + q < n_msgs ? crc32::segments_of(lens[base + q], kCrcSegment) : 0;
        mine += c[q];
    }
    uint64_t total;
    uint64_t at = block_scan_256(mine, buf, &total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (base + q < n_msgs) seg_first[base + q] = at;
        at += c[q];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums[0 .. n_blocks) -> their exclusive prefix sum, block_sums[n_blocks] = the total
__global__ __launch_bounds__(256) void crc32_plan_blocks_kernel(uint64_t* block_sums, uint64_t n_blocks) {
    __shared__ uint64_t buf[256];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_blocks; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < n_blocks ? block_sums[i] : 0;
        uint64_t total;
        const uint64_t ex = block_scan_256(v, buf, &total);
        if (i < n_blocks) block_sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) block_sums[n_blocks] = carry;
}

__global__ __launch_bounds__(256) void crc32_plan_add_kernel(uint64_t* seg_first, const uint64_t* block_sums, uint64_t n_msgs,
                                                             uint64_t n_blocks) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n_msgs) seg_first[i] += block_sums[i / kCrcPlanItems];
    else if (i == n_msgs) seg_first[i] = block_sums[n_blocks];
}

// ---- segments -----------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t R = kCrcTableReplicas;

// Entry e of table t for this lane.  ds_read_b32 banks are (address / 4) % 32 and conflicts count within a half wave:
// with R interleaved copies a lane reads bank (e * R + lane % R) % 32, so the 32 lanes of a half fall into R classes
// that can never meet, 32 / R lanes over 32 / R banks each.
__device__ __forceinline__ uint32_t tab(const uint32_t* lds, uint32_t t, uint32_t e, uint32_t rep) { return lds[(t * 256 + e) * R + rep]; }

// pure(16 bytes): slicing-by-8, twice
__device__ __forceinline__ uint32_t pure16(const uint32_t* lds, uint32_t rep, uint64_t lo, uint64_t hi) {
    uint32_t w0 = static_cast<uint32_t>(lo), w1 = static_cast<uint32_t>(lo >> 32);
    uint32_t s = tab(lds, 7, w0 & 255, rep) ^ tab(lds, 6, (w0 >> 8) & 255, rep) ^ tab(lds, 5, (w0 >> 16) & 255, rep) ^ tab(lds, 4, w0 >> 24, rep) ^
                 tab(lds, 3, w1 & 255, rep) ^ tab(lds, 2, (w1 >> 8) & 255, rep) ^ tab(lds, 1, (w1 >> 16) & 255, rep) ^ tab(lds, 0, w1 >> 24, rep);
    w0 = static_cast<uint32_t>(hi) ^ s; w1 = static_cast<uint32_t>(hi >> 32);
    return tab(lds, 7, w0 & 255, rep) ^ tab(lds, 6, (w0 >> 8) & 255, rep) ^ tab(lds, 5, (w0 >> 16) & 255, rep) ^ tab(lds, 4, w0 >> 24, rep) ^
           tab(lds, 3, w1 & 255, rep) ^ tab(lds, 2, (w1 >> 8) & 255, rep) ^ tab(lds, 1, (w1 >> 16) & 255, rep) ^ tab(lds, 0, w1 >> 24, rep);
}
// reg * x^(8 * 1024): tables 8..11
__device__ __forceinline__ uint32_t times_stride(const uint32_t* lds, uint32_t rep, uint32_t reg) {
    return tab(lds, 8, reg & 255, rep) ^ tab(lds, 9, (reg >> 8) & 255, rep) ^ tab(lds, 10, (reg >> 16) & 255, rep) ^ tab(lds, 11, reg >> 24, rep);
}

} // namespace

template <uint32_t POLY>
__global__ __launch_bounds__(256) void crc32_segments_kernel(const uint8_t* data, const uint64_t* offs, const uint64_t* lens,
                                                             const uint64_t* seg_first, uint64_t n_msgs, uint64_t total_segments,
                                                             uint64_t segs_per_wave, uint32_t* seg_pure) {
    __shared__ uint32_t lds[12 * 256 * R];
    {
        const uint32_t* src = &g_crc_tables.slice[0][0];    // slice[8][256] and stride[4][256] are adjacent: tables 0..11
        for (uint32_t i = threadIdx.x; i < 12 * 256 * R; i += 256) lds[i] = src[i / R];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t rep = lane & (R - 1);
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t s0 = wave * segs_per_wave;
    if (s0 >= total_segments) return;
    const uint64_t s1 = s0 + segs_per_wave < total_segments ? s0 + segs_per_wave : total_segments;
    // the message of segment s0: the last i with seg_first[i] <= s0 (counts are >= 1: seg_first is strictly increasing)
    uint64_t lo = 0, hi = n_msgs - 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (seg_first[mid] <= s0) lo = mid; else hi = mid - 1;
    }
    uint64_t msg = lo, first = seg_first[msg], next = seg_first[msg + 1];
    for (uint64_t s = s0; s < s1; ++s) {
        if (s == next) { ++msg; first = next; next = seg_first[msg + 1]; }
        const uint64_t len = lens[msg];
        const uint64_t at = (s - first) * kCrcSegment;
        const uint32_t seg_len = len - at < kCrcSegment ? static_cast<uint32_t>(len - at) : kCrcSegment;
        if (seg_len == 0) {         // (the one segment of an empty message)
            if (lane == 0) seg_pure[s] = 0;
            continue;
        }
        const uint64_t addr = reinterpret_cast<uint64_t>(data) + offs[msg] + at;
        const crc32::Granules g = crc32::granules_of(addr, seg_len);
        const uint4* gran = reinterpret_cast<const uint4*>(addr - g.head);
        // every load of the segment is issued before the first table look-up: body granules lane + 64 t (at most 256
        // of them: a segment spans 4 steps), and the partial tail granule on lane body % 64
        uint4 v[4];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
            if (t * 64 + lane < g.body) v[t] = gran[t * 64 + lane];
        const bool has_tail = g.tail != 0 && lane == (g.body & 63);
        uint4 tv = make_uint4(0, 0, 0, 0);
        if (has_tail) tv = gran[g.body];
        uint32_t reg = 0;
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
            if (t * 64 + lane < g.body) {
                uint64_t l64 = v[t].x | static_cast<uint64_t>(v[t].y) << 32, h64 = v[t].z | static_cast<uint64_t>(v[t].w) << 32;
                if (t == 0 && lane == 0 && g.head) {    // the bytes of granule 0 in front of the segment: leading zeros are free
                    const uint32_t hb = 8 * g.head;
                    if (hb >= 64) { l64 = 0; h64 &= ~0ull << (hb - 64); } else l64 &= ~0ull << hb;
                }
                reg = times_stride(lds, rep, reg) ^ pure16(lds, rep, l64, h64);
            }
        reg = crc32::mulmod<POLY>(reg, g_crc_tables.small[crc32::lane_final_shift(g, lane)]);
        if (has_tail) {
            uint64_t l64 = tv.x | static_cast<uint64_t>(tv.y) << 32, h64 = tv.z | static_cast<uint64_t>(tv.w) << 32;
            if (g.body == 0 && g.head) {                // a segment inside one granule: head and tail in the same one
                const uint32_t hb = 8 * g.head;
                if (hb >= 64) { l64 = 0; h64 &= ~0ull << (hb - 64); } else l64 &= ~0ull << hb;
            }
            // the tail's bytes move to the END of the granule (zero bytes in front are free, the bytes behind the segment fall off)
            const uint32_t sh = 8 * (16 - g.tail);
            if (sh >= 64) { h64 = l64 << (sh - 64); l64 = 0; } else { h64 = (h64 << sh) | (l64 >> (64 - sh)); l64 <<= sh; }
            reg ^= pure16(lds, rep, l64, h64);
        }
        reg = wave_xor(reg);
        if (lane == 0) seg_pure[s] = reg;
    }
}

// ---- fold ---------------------------------------------------------------------------------------------------------------
template <uint32_t POLY>
__global__ __launch_bounds__(256) void crc32_fold_kernel(const uint64_t* lens, const uint64_t* seg_first, const uint32_t* seg_pure,
                                                         uint64_t n_msgs, uint32_t* out) {
    __shared__ uint32_t op[4 * 256];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) op[i] = (&g_crc_tables.segment[0][0])[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t msg = static_cast<uint64_t>(blockIdx.x) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (msg >= n_msgs) return;
    const uint64_t len = lens[msg];
    const uint32_t* pure = seg_pure + seg_first[msg];
    const uint64_t full = len / kCrcSegment, rest = len - full * kCrcSegment;
    // lane l: full segments [l q, (l + 1) q); the initial value is the register in front of lane 0's run
    const uint64_t q = (full + 63) / 64;
    const uint64_t b = lane * q < full ? lane * q : full, e = b + q < full ? b + q : full;
    uint32_t reg = lane == 0 ? 0xFFFFFFFFu : 0u;
    for (uint64_t j = b; j < e; ++j)
        reg = op[reg & 255] ^ op[256 + ((reg >> 8) & 255)] ^ op[512 + ((reg >> 16) & 255)] ^ op[768 + (reg >> 24)] ^ pure[j];
    // ... which still has (full - e) segments and the partial one to travel: x^(8 m), m < 1024 from the table, the rest of
    // the length by square-and-multiply (x^(2^k), k from 13)
    if (reg) {
        const uint64_t after = (full - e) * kCrcSegment + rest;
        const uint32_t low = static_cast<uint32_t>(after) & (crc32::kSmallShifts - 1);
        if (low) reg = crc32::mulmod<POLY>(reg, g_crc_tables.small[low]);
        uint32_t k = 3 + crc32::kSmallShiftBits;
        for (uint64_t m = after >> crc32::kSmallShiftBits; m; m >>= 1, ++k)
            if (m & 1) reg = crc32::mulmod<POLY>(reg, g_crc_tables.pow2[k]);
    }
    reg = wave_xor(reg);
    if (lane == 0) out[msg] = ~(rest ? reg ^ pure[full] : reg);
}

// ---- compare (the model is digest_compare_kernel) -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crc32_compare_kernel(const uint32_t* actual, const uint32_t* expected, uint64_t n, uint8_t* valid,
                                                            unsigned long long* n_invalid) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        bad = actual[i] != expected[i];
        valid[i] = bad ? 0 : 1;
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_invalid, static_cast<unsigned long long>(__popcll(m)));
}

// =================================================================================================
// Launchers
// =================================================================================================
#define LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_crc32_chunk_table(hipStream_t st, const uint64_t* blob_off, const uint32_t* chunk_blob, const uint64_t* chunk_offset,
                                    const uint64_t* chunk_size, const uint8_t* select, uint64_t n, uint64_t* offs, uint64_t* lens) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(crc32_chunk_table_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, st, blob_off, chunk_blob,
                       chunk_offset, chunk_size, select, n, offs, lens);
    LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_crc32_plan(hipStream_t st, const uint64_t* lens, uint64_t n_msgs, uint64_t* seg_first, uint64_t* block_sums) {
    if (n_msgs == 0) return hipSuccess;
    const uint64_t nb = crc_plan_blocks(n_msgs);
    hipLaunchKernelGGL(crc32_plan_count_kernel, dim3(static_cast<uint32_t>(nb)), dim3(256), 0, st, lens, n_msgs, seg_first, block_sums);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(crc32_plan_blocks_kernel, dim3(1), dim3(256), 0, st, block_sums, nb);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(crc32_plan_add_kernel, dim3(static_cast<uint32_t>((n_msgs + 1 + 255) / 256)), dim3(256), 0, st, seg_first, block_sums,
                       n_msgs, nb);
    LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_crc32_segments(hipStream_t st, const uint8_t* data, const uint64_t* offs, const uint64_t* lens, const uint64_t* seg_first,
                                 uint64_t n_msgs, uint64_t total_segments, uint32_t n_cus, uint32_t* seg_pure) {
    if (n_msgs == 0 || total_segments == 0) return hipSuccess;
    // three workgroups of four waves per CU is what the tables' LDS allows; fewer waves than that when there is less work
    const uint64_t max_waves = static_cast<uint64_t>(n_cus ? n_cus : 256) * 12;
    const uint64_t waves = total_segments < max_waves ? total_segments : max_waves;
    const uint64_t blocks = (waves + 3) / 4;
    const uint64_t per_wave = (total_segments + blocks * 4 - 1) / (blocks * 4);
    hipLaunchKernelGGL(crc32_segments_kernel<kPoly>, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, st, data, offs, lens, seg_first, n_msgs,
                       total_segments, per_wave, seg_pure);
    LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_crc32_fold(hipStream_t st, const uint64_t* lens, const uint64_t* seg_first, const uint32_t* seg_pure, uint64_t n_msgs,
                             uint32_t* out) {
    if (n_msgs == 0) return hipSuccess;
    hipLaunchKernelGGL(crc32_fold_kernel<kPoly>, dim3(static_cast<uint32_t>((n_msgs + 3) / 4)), dim3(256), 0, st, lens, seg_first, seg_pure,
                       n_msgs, out);
    LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_crc32_compare(hipStream_t st, const uint32_t* actual, const uint32_t* expected, uint64_t n, uint8_t* valid,
                                unsigned long long* n_invalid) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(crc32_compare_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, st, actual, expected, n, valid, n_invalid);
    LAUNCH_CHECK();
    return hipSuccess;
}

} // namespace yams_accel
