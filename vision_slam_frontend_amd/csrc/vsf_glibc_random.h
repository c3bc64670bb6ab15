// vsf_glibc_random.h -- glibc's rand() (TYPE_3, the default: random_r.c), stated ONCE: the ObserveImage queue's colour kernel
// (k_draw.hip), the queue's host side (vsf_observe.hip seeds the streams' states) and the host classes' per-call drawing
// (host/slam_frontend.cc) all include this file, so a stream's colours are srand(seed) / rand() / rand() ... wherever they are
// drawn.  tests/cpp/test_glibc_random.cc holds it against the C library's srandom() / random() draw for draw.
//
//   state     31 words r[] and the position of the REAR pointer; the front pointer is 3 words ahead (SEP_3), both wrap at 31
//   a draw    r[front] += r[rear] in 32-bit ring arithmetic;  the draw is r[front] >> 1;  both pointers move on by one
//             (so r[i] = r[i - 31] + r[i - 3] along the sequence)
//   seeding   r[0] = seed (0 is taken as 1);  r[i] = 16807 r[i - 1] mod 2147483647 by Schrage's split
//             (hi = w / 127773, lo = w % 127773, w = 16807 lo - 2836 hi, + 2147483647 if negative), the words as int32;
//             rear = 0;  then 310 draws are thrown away
//   a colour  cv::Scalar(rand() % 255, rand() % 255, rand() % 255) (slam_frontend.cc:95) as GCC evaluates it: right to left,
//             the FIRST draw is channel 2;  packed b | g << 8 | r << 16
//
// Three draws in a row touch three different words (the lag is 3), and after 31 draws the rear pointer is back where it
// was: 93 draws -- 31 colours -- from a window whose rear pointer is 0 name every word by a constant.  colours31 is that
// block, for code that must keep the window in registers (a register array indexed by a runtime value goes to scratch on
// the GPU); next() is the same draw with the position as a value, for everything else.
#ifndef VSF_GLIBC_RANDOM_H_
#define VSF_GLIBC_RANDOM_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define VSF_RAND_FN __host__ __device__ __forceinline__
#else
#define VSF_RAND_FN inline
#endif

namespace vsfrand {

constexpr int kWords = 31, kSep = 3, kDiscard = 310;

struct State {
  uint32_t r[kWords];
  int32_t rear;  // [0, 31)
};
static_assert(sizeof(State) == 128, "31 words and a position: what the device keeps per stream");

// THE draw: the front word takes the rear word; the result is the new front word without its lowest bit.
VSF_RAND_FN uint32_t draw(uint32_t& front, uint32_t rear) {
  front += rear;
  return front >> 1;
}

VSF_RAND_FN uint32_t next(State& s) {
  const int f = s.rear + kSep >= kWords ? s.rear + kSep - kWords : s.rear + kSep;
  const uint32_t v = draw(s.r[f], s.r[s.rear]);
  s.rear = s.rear + 1 == kWords ? 0 : s.rear + 1;
  return v;
}

VSF_RAND_FN void seed(State& s, uint32_t seed_value) {
  int32_t w = (int32_t)(seed_value == 0 ? 1u : seed_value);
  s.r[0] = (uint32_t)w;
  for (int i = 1; i < kWords; i++) {
    const int32_t hi = w / 127773, lo = w % 127773;
    w = 16807 * lo - 2836 * hi;
    if (w < 0) w += 2147483647;
    s.r[i] = (uint32_t)w;
  }
  s.rear = 0;
  for (int i = 0; i < kDiscard; i++) (void)next(s);
}

// first, second, third: three draws in the order they were made
VSF_RAND_FN uint32_t pack_colour(uint32_t first, uint32_t second, uint32_t third) {
  return (third % 255u) | ((second % 255u) << 8) | ((first % 255u) << 16);
}

VSF_RAND_FN uint32_t next_colour(State& s) {
  const uint32_t a = next(s), b = next(s), c = next(s);
  return pack_colour(a, b, c);
}

// The next n (<= 31) colours of a window whose rear pointer is 0: emit(j, colour) for j in [0, n), every word named by a
// constant once the loop is unrolled.  Afterwards the rear pointer is (3 n) % 31.
template <class Emit>
VSF_RAND_FN void colours31(uint32_t (&r)[kWords], int n, Emit emit) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < kWords; j++) {
    if (j < n) {
      const uint32_t a = draw(r[(3 * j + 3) % kWords], r[(3 * j) % kWords]);
      const uint32_t b = draw(r[(3 * j + 4) % kWords], r[(3 * j + 1) % kWords]);
      const uint32_t c = draw(r[(3 * j + 5) % kWords], r[(3 * j + 2) % kWords]);
      emit(j, pack_colour(a, b, c));
    }
  }
}

// Where word i of a window whose rear pointer is `rear` goes when the window is rewritten with its rear pointer at 0.
VSF_RAND_FN int normalised_index(int i, int rear) { return i >= rear ? i - rear : i - rear + kWords; }

}  // namespace vsfrand

#endif  // VSF_GLIBC_RANDOM_H_
