// Stand-alone print-out of the bounds stage's public structs as include/rl_abi.h lays them out:
// one line per struct with its size, then one line per field with its offset and size.  It also
// writes and reads every field once through the struct, so a sanitizer build sees the layout
// used.  No HIP call; built and run by tests/test_bounds_layout_cpu.py, which compares the
// lines with the ctypes structures of abi.py.
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "rl_abi.h"

#define FIELD(S, f) std::printf("%s.%s %zu %zu\n", #S, #f, offsetof(S, f), sizeof(((S*)nullptr)->f))

int main() {
    std::printf("rl_bnd_query %zu\n", sizeof(rl_bnd_query));
    FIELD(rl_bnd_query, veh_width);
    FIELD(rl_bnd_query, margin);
    std::printf("rl_bnd %zu\n", sizeof(rl_bnd));
    FIELD(rl_bnd, lo);
    FIELD(rl_bnd, hi);
    FIELD(rl_bnd, nx);
    FIELD(rl_bnd, ny);
    std::printf("rl_hzn_bnd %zu\n", sizeof(rl_hzn_bnd));
    FIELD(rl_hzn_bnd, lo);
    FIELD(rl_hzn_bnd, hi);
    FIELD(rl_hzn_bnd, lo0);
    FIELD(rl_hzn_bnd, hi0);

    double cell[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    rl_bnd b;
    std::memset(&b, 0, sizeof(b));
    b.lo = cell; b.hi = cell + 1; b.nx = cell + 2; b.ny = cell + 3;
    rl_hzn_bnd h;
    std::memset(&h, 0, sizeof(h));
    h.lo = cell + 4; h.hi = cell + 5; h.lo0 = cell + 6; h.hi0 = cell + 7;
    const rl_bnd_query q = {1.25, 0.5};
    const double sum = *b.lo + *b.hi + *b.nx + *b.ny + *h.lo + *h.hi + *h.lo0 + *h.hi0 + q.veh_width + q.margin;
    if (sum != 29.75) {
        std::printf("bounds layout: fields overlap (sum %.17g)\n", sum);
        return 1;
    }
    std::printf("bounds layout ok\n");
    return 0;
}
