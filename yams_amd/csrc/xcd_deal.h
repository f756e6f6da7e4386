// xcd_deal.h — which 512-row unit is the j-th unit of row stream (st, xcd) of the resident-query int8 sweep.
//
// Shared by the kernels (scan_tiles_i8d_kernel, scan_tiles_i8r_kernel, prep_i8_kernel), their host code and a CPU test
// (tests/cpp/xcd_deal_test.cpp): plain C++, no HIP types.
//
// A launch has eight XCDs with `streams_x` row streams each (workgroup b runs on XCD b % 8; stream = st * 8 + xcd).  XCD x owns
// the contiguous unit range [off[x], off[x + 1]); its streams interleave inside it:
//
//     unit(st, xcd, j) = off[xcd] + st + j * streams_x        (the stream ends when that reaches off[xcd + 1])
//
// off[] comes from eight weights (Q16, 65536 = an equal share).  With equal weights XCD x gets exactly the units the former
// rule `stream + j * n_streams` gave its streams, and every stream the same length as before: n_units = q * n_streams + r
// gave stream s q + (s < r) units, XCD x therefore q * streams_x + c_x with c_x = #{st : st * 8 + x < r} — the streams
// with the extra unit are its lowest-numbered ones, which is what the interleave gives them.
//
// Unequal weights move units between XCDs: XCD x takes d_x = (n_units / 8) * e_x more than its equal share, e_x = its weight
// relative to the mean of the eight, clamped to +-XCD_DEAL_CLAMP (8 %) and then shrunk on the heavier side until the e_x sum to
// zero — so no XCD, and no stream, ever draws more than 8 % (+ one unit of rounding) beyond its equal share, which the survivor
// log's capacity (i8_log_capacity: four times a wave's share + 256) covers with room to spare.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XCD_DEAL_FN __host__ __device__ inline
#else
#define XCD_DEAL_FN inline
#endif

namespace yams_accel {

constexpr uint32_t XCD_DEAL_XCDS = 8;
constexpr uint32_t XCD_DEAL_ONE = 65536;      // weight of an equal share (Q16)
constexpr int32_t XCD_DEAL_CLAMP = 5242;      // floor(0.08 * 65536): the furthest a share moves from equal

// units of XCD x under the equal deal (= what `stream + j * n_streams` gave its streams_x streams)
XCD_DEAL_FN uint32_t xcd_deal_equal_count(uint32_t n_units, uint32_t streams_x, uint32_t x) {
    const uint32_t n_streams = streams_x * XCD_DEAL_XCDS;
    const uint32_t q = n_units / n_streams, r = n_units % n_streams;
    const uint32_t c = r > x ? (r - x + XCD_DEAL_XCDS - 1) / XCD_DEAL_XCDS : 0u; // #{st : st * 8 + x < r}
    return q * streams_x + (c < streams_x ? c : streams_x);
}

// e[x]: the relative move of XCD x's share (Q16, |e| <= XCD_DEAL_CLAMP, |sum| < 8: the rounding of the shrink)
XCD_DEAL_FN void xcd_deal_moves(const uint32_t* w, int32_t* e) {
    uint64_t sum = 0;
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) sum += w[x];
    int64_t pos = 0, neg = 0;
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) {
        int64_t v = sum ? static_cast<int64_t>((static_cast<uint64_t>(w[x]) * XCD_DEAL_XCDS * XCD_DEAL_ONE) / sum) - XCD_DEAL_ONE : 0;
        v = v > XCD_DEAL_CLAMP ? XCD_DEAL_CLAMP : (v < -XCD_DEAL_CLAMP ? -XCD_DEAL_CLAMP : v);
        e[x] = static_cast<int32_t>(v);
        if (v > 0) pos += v; else neg -= v;
    }
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) { // the heavier side shrinks to the lighter one's sum (towards zero: inside the clamp)
        if (pos > neg && e[x] > 0) e[x] = static_cast<int32_t>(static_cast<int64_t>(e[x]) * neg / pos);
        else if (neg > pos && e[x] < 0) e[x] = -static_cast<int32_t>(static_cast<int64_t>(-e[x]) * pos / neg);
    }
}

// off[0..8] from eight weights
XCD_DEAL_FN void xcd_deal_offsets(const uint32_t* w, uint32_t n_units, uint32_t streams_x, uint32_t* off) {
    int32_t e[XCD_DEAL_XCDS];
    xcd_deal_moves(w, e);
    int64_t cnt[XCD_DEAL_XCDS];
    int64_t rest = 0; // units the truncated moves leave over (a few)
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) {
        const int64_t d = static_cast<int64_t>(n_units) * e[x] / static_cast<int64_t>(XCD_DEAL_XCDS * XCD_DEAL_ONE); // (towards zero)
        cnt[x] = static_cast<int64_t>(xcd_deal_equal_count(n_units, streams_x, x)) + d;
        if (cnt[x] < 0) cnt[x] = 0;
        rest -= cnt[x];
    }
    rest += n_units;
    for (uint32_t x = 0; rest != 0; x = (x + 1) % XCD_DEAL_XCDS) { // one at a time, round the XCDs
        if (rest > 0) { ++cnt[x]; --rest; }
        else if (cnt[x] > 0) { --cnt[x]; ++rest; }
    }
    off[0] = 0;
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) off[x + 1] = off[x] + static_cast<uint32_t>(cnt[x]);
}

// the j-th unit of stream (st, xcd); 0xffffffff past the stream's end
XCD_DEAL_FN uint32_t xcd_deal_unit(uint32_t off_lo, uint32_t off_hi, uint32_t streams_x, uint32_t st, uint32_t j) {
    const uint64_t u = static_cast<uint64_t>(off_lo) + st + static_cast<uint64_t>(j) * streams_x;
    return u < off_hi ? static_cast<uint32_t>(u) : 0xffffffffu;
}

// units of stream (st, xcd)
XCD_DEAL_FN uint32_t xcd_deal_stream_length(uint32_t off_lo, uint32_t off_hi, uint32_t streams_x, uint32_t st) {
    const uint32_t n = off_hi - off_lo;
    return n > st ? (n - st + streams_x - 1) / streams_x : 0u;
}

// the most units a stream can get, whatever the weights: the clamp on top of the equal deal's longest stream (+ rounding)
XCD_DEAL_FN uint32_t xcd_deal_max_stream_length(uint32_t n_units, uint32_t streams_x) {
    const uint32_t n_streams = streams_x * XCD_DEAL_XCDS;
    const uint64_t xcd_most = static_cast<uint64_t>((n_units + n_streams - 1) / n_streams) * streams_x
                              + (static_cast<uint64_t>(n_units) * XCD_DEAL_CLAMP) / (XCD_DEAL_XCDS * XCD_DEAL_ONE) + 1u;
    return static_cast<uint32_t>((xcd_most + streams_x - 1) / streams_x);
}

// ---- feedback: what a finished filter launch says about the next one's weights ---------------------------------------------
// XCD x scored n[x] units in t[x] ticks (from the launch's first workgroup begin to the XCD's last wave end): its pace is
// n[x] / t[x], the share that would have made all eight end together is proportional to it.  The weights follow that share
// as a running average, a quarter of the way per launch: the end of one XCD moves by 0.5-2 % of the launch from one launch
// to the next while the differences between XCDs are 2-4 % (profiles/xcd_balance.json), so one launch alone is no guide.
// Weights stay inside the clamp.  A launch with an idle XCD or a nonsensical time teaches nothing.
XCD_DEAL_FN void xcd_deal_feedback(uint32_t* w, const uint32_t* n, const int64_t* t) {
    double rate[XCD_DEAL_XCDS], sum = 0.0;
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) {
        if (n[x] == 0 || t[x] <= 0) return;
        rate[x] = static_cast<double>(n[x]) / static_cast<double>(t[x]);
        sum += rate[x];
    }
    const double lo = static_cast<double>(XCD_DEAL_ONE - XCD_DEAL_CLAMP), hi = static_cast<double>(XCD_DEAL_ONE + XCD_DEAL_CLAMP);
    for (uint32_t x = 0; x < XCD_DEAL_XCDS; ++x) {
        double target = rate[x] * XCD_DEAL_XCDS / sum * XCD_DEAL_ONE;
        target = target < lo ? lo : (target > hi ? hi : target);
        double v = static_cast<double>(w[x]);
        v = v < lo ? lo : (v > hi ? hi : v);
        v += (target - v) * 0.25;
        w[x] = static_cast<uint32_t>(v + 0.5);
    }
}

// ---- the per-context table (device memory, uint32 words) ----------------------------------------------------------------------
constexpr uint32_t XCD_TABLE_WEIGHTS = 0;       // [8]  running weights (Q16)
constexpr uint32_t XCD_TABLE_OFF_FILTER = 8;    // [9]  off[] of the filter launch
constexpr uint32_t XCD_TABLE_OFF_SAMPLE = 17;   // [9]  off[] of a sample pass in the resident form (the same weights, its own unit count)
constexpr uint32_t XCD_TABLE_TICKS = 32;        // [n_streams * n_qt][9]  per workgroup (stream * n_qt + qt): begin, end of waves 0..7; 0 = not written
constexpr uint32_t XCD_TICKS_PER_WG = 9;

// what prep_i8_kernel gets: the table, the plan of this batch's two launches, and where the weights come from
enum { XCD_DEAL_FEEDBACK = 0, XCD_DEAL_RESET = 1, XCD_DEAL_FORCED = 2 };
struct XcdDealPrep { uint32_t* table; uint32_t n_units_filter, n_units_sample, streams_x, n_qt, mode; uint32_t forced[8]; };

} // namespace yams_accel
