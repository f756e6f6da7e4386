// pq_host_avx2_a.cpp — a table sum the way an AVX2 host writes it (compiled with -mavx2, linked into pq_calibration_test):
// eight gathered table entries per step into one accumulator register, the register reduced with extract-high + add, movehl
// + add, shuffle + add, then the m % 8 tail elements one by one.  The probe must call it x8_halves_tail.
#include <immintrin.h>

#include <cstddef>
#include <cstdint>

extern "C" float pq_host_avx2_halves(const float* table, const uint8_t* code, size_t m) {
    const __m256i step = _mm256_setr_epi32(0, 256, 512, 768, 1024, 1280, 1536, 1792);
    __m256 acc = _mm256_setzero_ps();
    size_t j = 0;
    for (; j + 8 <= m; j += 8) {
        const __m128i c8 = _mm_loadl_epi64(reinterpret_cast<const __m128i*>(code + j));
        const __m256i idx = _mm256_add_epi32(_mm256_cvtepu8_epi32(c8), step);
        acc = _mm256_add_ps(acc, _mm256_i32gather_ps(table + j * 256, idx, 4));
    }
    const __m128 s4 = _mm_add_ps(_mm256_castps256_ps128(acc), _mm256_extractf128_ps(acc, 1));   // p[l] + p[l + 4]
    const __m128 s2 = _mm_add_ps(s4, _mm_movehl_ps(s4, s4));                                      // [0] + [2], [1] + [3]
    const __m128 s1 = _mm_add_ss(s2, _mm_shuffle_ps(s2, s2, 1));                                  // [0] + [1]
    float s = _mm_cvtss_f32(s1);
    for (; j < m; ++j) s += table[j * 256 + code[j]];
    return s;
}
