// The owner template of csrc/vsf_own.h (every device buffer, pinned buffer, event and stream of the library is one of its four
// instances) with traits that count: each handle that is acquired is released exactly once, and never when it was handed out.
// Built with -fsanitize=address,undefined by tests/test_own.py; prints "ok <acquired>" or the first failed check.
#define VSF_OWN_NO_HIP
#include "../../vision_slam_frontend_amd/csrc/vsf_own.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

namespace {

int g_acquired = 0, g_released = 0;
std::map<long, int> g_release_count;  // per handle

struct CountTraits {
  using handle = long*;  // (never dereferenced: the handle's value is its serial number)
  static int acquire(handle* h, int fail = 0) {
    if (fail) return fail;
    *h = reinterpret_cast<handle>((long)++g_acquired * 8);
    return 0;
  }
  static void release(handle h) {
    g_released++;
    g_release_count[reinterpret_cast<long>(h)]++;
  }
};
using Own = vsfi::Owned<CountTraits>;

#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);   \
      std::exit(1);                                        \
    }                                                      \
  } while (0)

int released(const long* h) { return g_release_count[reinterpret_cast<long>(h)]; }

struct Queue {  // a struct of owners, as vsf_ctx::Observe is
  Own a, b[3];
  std::vector<Own> v;
  int depth = 0;
};

}  // namespace

int main() {
  {  // an empty owner releases nothing
    Own e;
    CHECK(!e && e.get() == nullptr);
    e.reset();
  }
  CHECK(g_released == 0);
  {  // move construction leaves the source empty
    Own a;
    CHECK(a.alloc() == 0);
    long* h = a;
    Own b(std::move(a));
    CHECK(a.get() == nullptr && b.get() == h && released(h) == 0);
  }
  CHECK(g_acquired == 1 && g_released == 1);
  {  // move assignment releases the target's old handle exactly once; self-move keeps the handle
    Own a, b;
    CHECK(a.alloc() == 0 && b.alloc() == 0);
    long *ha = a, *hb = b;
    b = std::move(a);
    CHECK(released(hb) == 1 && released(ha) == 0 && b.get() == ha && a.get() == nullptr);
    Own& same = b;
    b = std::move(same);
    CHECK(b.get() == ha && released(ha) == 0);
  }
  CHECK(g_acquired == 3 && g_released == 3);
  {  // alloc() over a held handle releases the old one first; a failed alloc() leaves the owner empty
    Own a;
    CHECK(a.alloc() == 0);
    long* h0 = a;
    CHECK(a.alloc() == 0);
    CHECK(released(h0) == 1 && a.get() != h0);
    long* h1 = a;
    CHECK(a.alloc(7) == 7 && released(h1) == 1 && !a);
  }
  CHECK(g_acquired == 5 && g_released == 5);
  {  // reset() releases once, and the destructor then releases nothing
    Own a;
    CHECK(a.alloc() == 0);
    long* h = a;
    a.reset();
    CHECK(released(h) == 1 && !a);
  }
  CHECK(g_acquired == 6 && g_released == 6);
  long* handed_out = nullptr;
  {  // release() returns the handle, and no release follows
    Own a;
    CHECK(a.alloc() == 0);
    long* h = a;
    handed_out = a.release();
    CHECK(handed_out == h && !a);
  }
  CHECK(g_acquired == 7 && g_released == 6 && released(handed_out) == 0);
  {  // ... until somebody adopts it (the retired list)
    Own adopted(handed_out);
  }
  CHECK(g_released == 7 && released(handed_out) == 1);
  {  // a vector of owners, pushed past several reallocations and then cleared
    std::vector<Own> v;
    std::vector<long*> hs;
    size_t reallocations = 0, cap = v.capacity();
    for (int i = 0; i < 100; i++) {
      v.emplace_back();
      CHECK(v.back().alloc() == 0);
      hs.push_back(v.back());
      if (v.capacity() != cap) reallocations++, cap = v.capacity();
    }
    CHECK(reallocations >= 4);
    for (long* h : hs) CHECK(released(h) == 0);
    v.clear();
    for (long* h : hs) CHECK(released(h) == 1);
  }
  CHECK(g_acquired == 107 && g_released == 107);
  {  // a struct of owners assigned from a default-constructed one releases all of its handles (o = Observe())
    Queue q;
    std::vector<long*> hs;
    CHECK(q.a.alloc() == 0);
    hs.push_back(q.a);
    for (Own& o : q.b) {
      CHECK(o.alloc() == 0);
      hs.push_back(o);
    }
    for (int i = 0; i < 5; i++) {
      q.v.emplace_back();
      CHECK(q.v.back().alloc() == 0);
      hs.push_back(q.v.back());
    }
    q.depth = 4;
    q = Queue();
    for (long* h : hs) CHECK(released(h) == 1);
    CHECK(!q.a && !q.b[2] && q.v.empty() && q.depth == 0);
  }
  // at exit: releases equal acquisitions, no handle released twice
  CHECK(g_acquired == 116 && g_released == g_acquired);
  for (const auto& kv : g_release_count) CHECK(kv.second == 1);
  std::printf("ok %d\n", g_acquired);
  return 0;
}
