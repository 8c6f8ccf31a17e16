// The stand-alone program of tests/test_item_magic.py: item_magic.h evaluated by the host
// compiler (it may be built with -fsanitize=address,undefined and run on its own).
//   item_magic_check eval D NMAX N...      -> "mul shift exact", then "q r" per numerator N
//   item_magic_check sweep D NMAX LO HI    -> "mismatches first" over every n in [LO, HI]
//   item_magic_check frame SPP SAMPLES TILES_X BAND NPIX MAX_SAMPLES ROWS W H X0 Y0
//                                          -> "on div_ok pow2 spp_log2"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "item_magic.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const auto u64 = [&](int k) { return (uint64_t)strtoull(argv[k], nullptr, 10); };
    if (!strcmp(argv[1], "frame") && argc == 13) {
        const yrt::item_magic m =
            yrt::make_item_magic((int)u64(2), (int)u64(3), (int)u64(4), (int)u64(5), u64(6), u64(7), u64(8),
                                 atoi(argv[9]), atoi(argv[10]), atoi(argv[11]), atoi(argv[12]));
        printf("%d %d %d %d\n", m.on, m.div_ok, m.pow2, m.spp_log2);
        return 0;
    }
    const uint32_t d = (uint32_t)u64(2);
    const yrt::udiv_magic g = yrt::make_udiv_magic(d, u64(3));
    if (!strcmp(argv[1], "eval")) {
        printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", g.mul, g.shift, g.exact);
        for (int k = 4; k < argc; k++) {
            const uint32_t n = (uint32_t)u64(k), q = yrt::magic_div(n, g);
            printf("%" PRIu32 " %" PRIu32 "\n", q, n - q * d);
        }
        return 0;
    }
    if (!strcmp(argv[1], "sweep") && argc == 6 && d != 0) {
        uint64_t bad = 0, first = 0;
        for (uint64_t n = u64(4); n <= u64(5); n++) {
            const uint32_t q = yrt::magic_div((uint32_t)n, g);
            if (q != (uint32_t)n / d || (uint32_t)n - q * d != (uint32_t)n % d) {
                if (!bad) first = n;
                bad++;
            }
        }
        printf("%" PRIu64 " %" PRIu64 "\n", bad, first);
        return 0;
    }
    return 2;
}
