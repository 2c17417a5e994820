// Tile geometry and the K-index map of the 7x7 / 2 stem kernels (conv_stem.hip): which LDS word of the parity-de-interleaved input
// tile tap k = (ci * 7 + ky) * 7 + kx of an output pixel reads.  Plain C++ (no HIP headers), so that the host test
// tests/emul/stem_map_emul.cpp compiles THIS code with g++ and tests/test_conv_stem_cpu.py replays both GEMMs through it in numpy.
#pragma once

#if defined(__HIPCC__)
#define STEM_HD __host__ __device__
#else
#define STEM_HD
#endif

namespace cd {

constexpr int STEM_PW = 36, STEM_RS = 2 * STEM_PW;   // words per parity run (32 pixels + 3 taps, padded) and per tile row
constexpr int SF_TY = 8, SF_ROWS = 2 * SF_TY + 5;    // forward: output rows per tile, input rows it reads
constexpr int SW_TY = 4, SW_ROWS = 2 * SW_TY + 5;    // weight gradient

STEM_HD constexpr int stem_k(int cin) { return cin * 49; }
STEM_HD constexpr int sf_ksteps(int cin) { return (cin * 49 + 15) / 16; }              // forward: K padded to the 16-tap MFMA step
STEM_HD constexpr int stem_kp(int cin) { return (cin * 49 + 31) / 32 * 32; }           // weight gradient: whole 32-tap column tiles
STEM_HD constexpr int stem_copad(int cout) { return cout <= 32 ? 32 : (cout + 63) / 64 * 64; }

// The tile starts at input (2 Y0 - 3, 2 X0 - 4); tile column c of row r of channel ci is word (ci * rows + r) * STEM_RS + (c & 1) * STEM_PW + c / 2.
STEM_HD constexpr int stem_tile_word(int ci, int r, int c, int rows) { return (ci * rows + r) * STEM_RS + (c & 1) * STEM_PW + (c >> 1); }
// LDS word of tap k relative to (tile row 2y, word i) of output pixel (Y0 + y, X0 + i): tile row 2y + ky, tile column 2i + kx + 1
STEM_HD constexpr int stem_off(int k, int rows) {
    const int ci = k / 49, t = k - ci * 49, ky = t / 7, kx = t - ky * 7;
    return stem_tile_word(ci, ky, kx + 1, rows);
}

}  // namespace cd
