// TEST INFRASTRUCTURE ONLY -- standalone AddressSanitizer/UBSan driver of the
// host emulation's step program with the speculative draw words
// (cotix_emu_scanspec.cpp emu_step_scanspec: the draw-word producer and the
// scan's round 0): keyl1_asan_driver.cpp's main, file formats and exit codes,
// with that entry point in place of emu_step_keyl1.
#define emu_step_keyl1 emu_step_scanspec
#include "keyl1_asan_driver.cpp"
