// pq_host_avx2_b.cpp — the other common end of an AVX2 table sum (compiled with -mavx2, linked into pq_calibration_test): the
// accumulator register reduced with extract-high + add, then movehdup + add (neighbours), movehl + add, then the m % 8 tail
// elements one by one.  The probe must call it x8_halves4_pairs_tail.
#include <immintrin.h>

#include <cstddef>
#include <cstdint>

extern "C" float pq_host_avx2_halves4_pairs(const float* table, const uint8_t* code, size_t m) {
    const __m256i step = _mm256_setr_epi32(0, 256, 512, 768, 1024, 1280, 1536, 1792);
    __m256 acc = _mm256_setzero_ps();
    size_t j = 0;
    for (; j + 8 <= m; j += 8) {
        const __m128i c8 = _mm_loadl_epi64(reinterpret_cast<const __m128i*>(code + j));
        const __m256i idx = _mm256_add_epi32(_mm256_cvtepu8_epi32(c8), step);
        acc = _mm256_add_ps(acc, _mm256_i32gather_ps(table + j * 256, idx, 4));
    }
    const __m128 s4 = _mm_add_ps(_mm256_castps256_ps128(acc), _mm256_extractf128_ps(acc, 1));   // p[l] + p[l + 4]
    const __m128 pairs = _mm_add_ps(s4, _mm_movehdup_ps(s4));                                     // [0] + [1], -, [2] + [3], -
    const __m128 one = _mm_add_ss(pairs, _mm_movehl_ps(pairs, pairs));                            // ([0] + [1]) + ([2] + [3])
    float s = _mm_cvtss_f32(one);
    for (; j < m; ++j) s += table[j * 256 + code[j]];
    return s;
}
