// csrc/vsf_glibc_random.h against the C library: srandom(seed) / random() draw for draw, next_colour against three draws in
// the reference's order, and colours31 -- the block the GPU kernel runs -- against next_colour for every count, followed by the
// rewrite of the window to rear pointer 0.  `colours SEED N` prints N packed colours (tests/test_glibc_random.py holds them
// against draw_ref.rand_colours).  Built plain and under ASan / UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vision_slam_frontend_amd/csrc/vsf_glibc_random.h"

static int fail(const char* what, unsigned seed, long i) {
  std::printf("FAIL %s seed %u draw %ld\n", what, seed, i);
  return 1;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "colours") == 0) {
    vsfrand::State s;
    vsfrand::seed(s, (uint32_t)std::strtoul(argv[2], nullptr, 0));
    for (long i = 0, n = std::atol(argv[3]); i < n; i++) std::printf("%u\n", vsfrand::next_colour(s));
    return 0;
  }
  const unsigned seeds[] = {0u, 1u, 2u, 7u, 4242u, 0xFFFFFFFFu};
  const long kDraws = 100000;
  long checked = 0;
  for (unsigned seed : seeds) {
    vsfrand::State s;
    vsfrand::seed(s, seed);
    srandom(seed);
    for (long i = 0; i < kDraws; i++, checked++)
      if ((long)vsfrand::next(s) != random()) return fail("next", seed, i);
    // rand() is random() in glibc: the colours are three draws each, the first one channel 2
    vsfrand::State a, b;
    vsfrand::seed(a, seed);
    vsfrand::seed(b, seed);
    for (long i = 0; i < 1000; i++) {
      const uint32_t c2 = vsfrand::next(b) % 255u, c1 = vsfrand::next(b) % 255u, c0 = vsfrand::next(b) % 255u;
      if (vsfrand::next_colour(a) != (c0 | (c1 << 8) | (c2 << 16))) return fail("next_colour", seed, i);
    }
    // the unrolled block: frames of every size 0 .. 100 in a row (blocks of 31 and a rest), the window rewritten to rear
    // pointer 0 after each frame, as the kernel does it
    vsfrand::State ref;
    vsfrand::seed(ref, seed);
    uint32_t win[vsfrand::kWords];
    for (int i = 0; i < vsfrand::kWords; i++) win[vsfrand::normalised_index(i, ref.rear)] = ref.r[i];
    for (int frame = 0; frame <= 100; frame++) {
      std::vector<uint32_t> got((size_t)frame, 0u);
      for (int base = 0; base < frame; base += vsfrand::kWords) {
        const int n = frame - base < vsfrand::kWords ? frame - base : vsfrand::kWords;
        vsfrand::colours31(win, n, [&](int j, uint32_t c) { got[(size_t)(base + j)] = c; });
      }
      const int rear = (3 * frame) % vsfrand::kWords;
      uint32_t tmp[vsfrand::kWords];
      for (int i = 0; i < vsfrand::kWords; i++) tmp[vsfrand::normalised_index(i, rear)] = win[i];
      std::memcpy(win, tmp, sizeof(win));
      for (int i = 0; i < frame; i++)
        if (got[(size_t)i] != vsfrand::next_colour(ref)) return fail("colours31", seed, frame * 1000L + i);
      for (int i = 0; i < vsfrand::kWords; i++)
        if (win[vsfrand::normalised_index(i, ref.rear)] != ref.r[i]) return fail("window", seed, frame);
    }
  }
  // seed 0 is seed 1
  vsfrand::State z, o;
  vsfrand::seed(z, 0);
  vsfrand::seed(o, 1);
  if (std::memcmp(&z, &o, sizeof(z)) != 0) return fail("seed 0", 0, 0);
  std::printf("ok %ld draws\n", checked);
  return 0;
}
