// crc32_launch.h — host-visible launch descriptors for crc32_kernels.hip (the batched CRC-32 of DESIGN 3.12).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/yams_mi355x_accel.h"

namespace yams_accel {

constexpr uint32_t kCrcSegment = YAMS_CRC32_SEGMENT_BYTES;
constexpr uint32_t kCrcPlanItems = 1024;    // messages one workgroup of the plan pass counts and scans
// static LDS of the kernels (tests/test_crc32_cpu.py holds the gfx950 metadata to these numbers)
constexpr uint32_t kCrcTableReplicas = 4;   // copies of every 256-entry table of the segment pass, interleaved entry by entry
constexpr uint32_t kCrcSegmentLds = 12 * 256 * 4 * kCrcTableReplicas;   // 8 slicing tables + 4 of the stride operator
constexpr uint32_t kCrcFoldLds = 4 * 256 * 4;                           // the segment operator
constexpr uint32_t kCrcPlanLds = 256 * 8;                               // one scan buffer

inline uint64_t crc_plan_blocks(uint64_t n_msgs) { return (n_msgs + kCrcPlanItems - 1) / kCrcPlanItems; }

// chunk i of an ingest result -> message i: offs[i] = blob_off[chunk_blob[i]] + chunk_offset[i], lens[i] = chunk_size[i],
// or 0 where select is given and select[i] == 0 (its bytes are then never read and its CRC is that of the empty message)
hipError_t launch_crc32_chunk_table(hipStream_t st, const uint64_t* blob_off, const uint32_t* chunk_blob, const uint64_t* chunk_offset,
                                    const uint64_t* chunk_size, const uint8_t* select, uint64_t n, uint64_t* offs, uint64_t* lens);
// seg_first[n_msgs + 1]: the exclusive prefix sum of the messages' segment counts (an empty message counts one);
// seg_first[n_msgs] is the total.  block_sums: crc_plan_blocks(n_msgs) + 1 words of scratch.
hipError_t launch_crc32_plan(hipStream_t st, const uint64_t* lens, uint64_t n_msgs, uint64_t* seg_first, uint64_t* block_sums);
// seg_pure[s] = the raw (no initial value, no final xor) CRC register of segment s, for every segment of every message
hipError_t launch_crc32_segments(hipStream_t st, const uint8_t* data, const uint64_t* offs, const uint64_t* lens, const uint64_t* seg_first,
                                 uint64_t n_msgs, uint64_t total_segments, uint32_t n_cus, uint32_t* seg_pure);
// out[i] = the finalised CRC-32 of message i
hipError_t launch_crc32_fold(hipStream_t st, const uint64_t* lens, const uint64_t* seg_first, const uint32_t* seg_pure, uint64_t n_msgs,
                             uint32_t* out);
hipError_t launch_crc32_compare(hipStream_t st, const uint32_t* actual, const uint32_t* expected, uint64_t n, uint8_t* valid,
                                unsigned long long* n_invalid);

} // namespace yams_accel
