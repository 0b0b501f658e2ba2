// The host plan of the wide stream banks (tests/test_fbank_bank_host.py).  Without arguments this is
// tests/bank_plan_driver.cpp, case for case: that file's main, included here under another name, so the rows of 65 .. 128
// floats go through the very lines the narrow ones go through.  With the argument `tiles` it prints what
// mfcc_amd/csrc/bank_plan.hpp makes of the delta kernels' tiles: first the line
//   kLdsFloats kWideLdsFloats kNarrowWidth
// then for every width 1 .. 128, order 1 .. 2, window 1 .. 8 the line
//   width order window tile_rows wide_tile_rows delta_tile_rows
// (Renaming that file's main this way leaves it unedited, and holds only while its main takes no arguments and the word
// `main` stands nowhere else in it: should that change, this driver has to take over its loop.)
#define main plan_cases
#include "bank_plan_driver.cpp"
#undef main

int main(int argc, char **argv) {
    if (argc < 2 || strcmp(argv[1], "tiles")) return plan_cases();
    using namespace mfcc_online;
    printf("%d %d %d\n", kLdsFloats, kWideLdsFloats, kNarrowWidth);
    for (int w = 1; w <= 128; ++w)
        for (int order = 1; order <= 2; ++order)
            for (int window = 1; window <= 8; ++window)
                printf("%d %d %d %d %d %d\n", w, order, window, tile_rows(w, order, window), wide_tile_rows(w, order, window),
                       delta_tile_rows(w, order, window));
    return 0;
}
