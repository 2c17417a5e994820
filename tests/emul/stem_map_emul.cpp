// Prints the K-index map of consistent_depth_amd/csrc/conv_stem_map.h for tests/test_conv_stem_cpu.py: one line of constants, then
// per (pass, cin) the LDS word offset of every tap, padding columns included as -1.
#include <cstdio>

#include "conv_stem_map.h"

int main() {
    using namespace cd;
    std::printf("CONST %d %d %d %d %d %d\n", STEM_PW, STEM_RS, SF_TY, SF_ROWS, SW_TY, SW_ROWS);
    for (int cin = 1; cin <= 4; ++cin) {
        std::printf("FWD %d %d", cin, sf_ksteps(cin) * 16);
        for (int k = 0; k < sf_ksteps(cin) * 16; ++k) std::printf(" %d", k < stem_k(cin) ? stem_off(k, SF_ROWS) : -1);
        std::printf("\nWGRAD %d %d", cin, stem_kp(cin));
        for (int k = 0; k < stem_kp(cin); ++k) std::printf(" %d", k < stem_k(cin) ? stem_off(k, SW_ROWS) : -1);
        std::printf("\n");
    }
    for (int c = 0; c < 72; ++c) std::printf("TILE %d %d\n", c, stem_tile_word(0, 0, c, 1));
    return 0;
}
