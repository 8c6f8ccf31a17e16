// item_magic.h -- unsigned division by a per-frame constant as a multiply-high and two shifts,
// for the index arithmetic of the item paths (wavefront.hip: pixel_of, primary_samples,
// sum_pixels). hipcc's n / d on a runtime d is a v_rcp_iflag_f32 sequence of 25-30 VALU
// instructions; the divisors here (spp, samples, tiles_x, band) are fixed for a frame.
//
// The round-up method, for numerators below 2^31 (every index of a frame whose pixels are
// counted in 32 bits is: a chunk's samples and a window's rows are ints, a tile index is a
// pixel index / 64): with s = floor(log2 d) and k = 32 + s,
//   m = ceil(2^k / d)  (< 2^32 for a d that is no power of two),  e = m d - 2^k  (0 < e < d),
//   floor(n m / 2^k) = floor(n / d)  iff  n e < (d - n mod d) 2^k,
// and n e < 2^31 2^(s + 1) = 2^k holds for every n < 2^31: the pair is exact on that whole
// range. The product is taken of 2 n, q = mulhi(2 n, m) >> (s + 1), so that a power of two,
// d = 2^s, fits the same form with m = 2^31 and the shift s. From n = 2^31 on 2 n wraps and
// the quotient is wrong for every d <= n: a pair asked for such an nmax (or for a divisor of
// 0 or above 2^31) says so in `exact`, and the callers keep the general division
// (item_magic::on). No host-accepted frame of fewer than 2^32 pixels is such a case.
//
// Plain C++: the host fills the pairs (run()), the kernels and tests/test_item_magic.py's
// stand-alone program evaluate them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define YRT_MAGIC_HD __host__ __device__ __forceinline__
#else
#define YRT_MAGIC_HD inline
#endif

namespace yrt {

constexpr uint32_t magic_nmax = 0x7fffffffu;  // the largest numerator a pair can be exact for

struct udiv_magic {
    uint32_t mul;    // ceil(2^(32 + floor(log2 d)) / d); 2^31 for a power of two
    uint32_t shift;  // of mulhi(2 n, mul): floor(log2 d) + 1; log2 d for a power of two
    uint32_t d;      // the divisor
    uint32_t exact;  // 1: the pair gives floor(n / d) for every n in [0, nmax]
};

// the pair of divisor d for numerators in [0, nmax]
YRT_MAGIC_HD udiv_magic make_udiv_magic(uint32_t d, uint64_t nmax) {
    udiv_magic g = {0u, 0u, d, 0u};
    if (d == 0u || d > 0x80000000u) return g;
    uint32_t s = 0;
    while (s < 31u && (2u << s) <= d) s++;  // 2^s <= d < 2^(s + 1)
    g.exact = nmax <= magic_nmax ? 1u : 0u;
    if ((d & (d - 1u)) == 0u) {
        g.mul = 0x80000000u, g.shift = s;
    } else {
        // floor(2^k / d) + 1 (d does not divide 2^k; 2^s < d, so the quotient is below 2^32)
        g.mul = (uint32_t)(((1ull << s) << 32) / d + 1u), g.shift = s + 1u;
    }
    return g;
}

YRT_MAGIC_HD uint32_t magic_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// floor(n / d) for n in the pair's range, from the pair's two words
YRT_MAGIC_HD uint32_t magic_div(uint32_t n, uint32_t mul, uint32_t shift) { return magic_mulhi(n << 1, mul) >> shift; }
YRT_MAGIC_HD uint32_t magic_div(uint32_t n, const udiv_magic& g) { return magic_div(n, g.mul, g.shift); }

// the divisors of a frame's item paths and what run() decides once for the whole frame
struct item_magic {
    udiv_magic spp;      // sample index of the chunk -> pixel of the chunk
    udiv_magic samples;  // sample of the pixel -> jj (and ii as the remainder)
    udiv_magic tiles_x;  // tile -> tile row (and column)
    udiv_magic band;     // local row -> band (and row in the band)
    int on;              // 1: every pair is exact and the frame's pixels are counted in 32 bits
    int div_ok;          // 1: camera_ray_w's divisions are in div_nr's range for every sample
    int pow2;            // 1: on, and 64 % spp == 0 -- an item's samples lie in one 8x8 tile
    int spp_log2;        // (pow2) log2 spp; samples is its square root, 1 << (spp_log2 / 2)
};

// npix_total: the frame's pixels in tile enumeration order (whole 8x8 tiles); max_samples: the
// most samples a chunk holds; rows: the local rows of those tiles. The camera's divisions --
// (ii + 0.5) / samples, u / width and v / height with u in [i, i + 1], i >= 0, never zero --
// are within div_nr's [2^-60, 2^60] for any positive int samples, width and height.
YRT_MAGIC_HD item_magic make_item_magic(int spp, int samples, int tiles_x, int band, uint64_t npix_total,
                                        uint64_t max_samples, uint64_t rows, int width, int height, int x0, int y0) {
    item_magic m = {};
    if (spp >= 1 && samples >= 1 && tiles_x >= 1 && band >= 1 && npix_total <= 0xffffffffull) {
        m.spp = make_udiv_magic((uint32_t)spp, max_samples);
        m.samples = make_udiv_magic((uint32_t)samples, (uint64_t)spp);
        m.tiles_x = make_udiv_magic((uint32_t)tiles_x, npix_total / 64u);
        m.band = make_udiv_magic((uint32_t)band, rows);
        m.on = (m.spp.exact & m.samples.exact & m.tiles_x.exact & m.band.exact) ? 1 : 0;
    }
    m.div_ok = samples >= 1 && width >= 1 && height >= 1 && x0 >= 0 && y0 >= 0;
    if (m.on && 64 % spp == 0 && samples * samples == spp) {
        m.pow2 = 1;
        while ((2 << m.spp_log2) <= spp) m.spp_log2++;
    }
    return m;
}

}  // namespace yrt
