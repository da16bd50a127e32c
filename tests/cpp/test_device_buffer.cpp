// test_device_buffer.cpp -- device-free: the owner of the library's device memory (sxmc_amd/csrc/device_buffer.h) over a
// host policy that allocates with malloc, logs every call, keeps the set of live blocks and fails the k-th allocation on
// demand.  What cannot be provoked on a GPU -- an allocation that fails in the middle of a creation or of a
// free-then-allocate -- is swept here: nothing leaks, nothing is freed twice, capacity is never ahead of the pointer.
#include "../../sxmc_amd/csrc/device_buffer.h"

#include <cstdlib>
#include <exception>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "mini_test.h"

namespace {

struct Heap {
  std::string calls;            // 'A' per allocate, 'F' per free, in order
  std::set<void*> live;
  int nalloc = 0, fail_at = 0;  // fail_at = k: the k-th allocate from now fails (0: none)
  int bad_frees = 0;            // frees of a block that is not live (double frees)
  void fresh(int k = 0) {
    calls.clear();
    nalloc = 0;
    fail_at = k;
  }
};
Heap heap;

struct HostMem {
  static int allocate(void** p, size_t bytes) {
    heap.calls += 'A';
    if (++heap.nalloc == heap.fail_at) return 2;   // (*p untouched, like a failed allocation of the runtime)
    *p = std::malloc(bytes ? bytes : 1);
    heap.live.insert(*p);
    return 0;
  }
  static int free(void* p) {
    heap.calls += 'F';
    if (!heap.live.erase(p)) {
      heap.bad_frees++;
      return 1;
    }
    std::free(p);
    return 0;
  }
};
template <typename T>
using Buf = sxbuf::Buffer<T, HostMem>;

// every scenario ends with nothing live and nothing freed twice
struct Clean {
  Clean() { heap = Heap{}; }
  ~Clean() noexcept(false) {
    if (std::uncaught_exceptions()) return;   // (a check above has failed already)
    EXPECT_EQ(heap.live.size(), 0u);
    EXPECT_EQ(heap.bad_frees, 0);
  }
};

// four buffers filled in sequence, early return on the first failure: the shape of sxmc_group_create (alloc into a
// handle held by a unique_ptr) and of sxmc_kde_set_eval_points (grow-only members of a living handle)
struct Four {
  Buf<int> a;
  Buf<float> b;
  Buf<double> c;
  Buf<void> d;
  size_t owned() const { return (size_t)!a.empty() + !b.empty() + !c.empty() + !d.empty(); }
  int fill(size_t n) {
    if (int rc = a.grow(n)) return rc;
    if (int rc = b.grow(2 * n)) return rc;
    if (int rc = c.grow(n + n / 4)) return rc;
    if (int rc = d.grow(16 * n)) return rc;
    return 0;
  }
};

int create_four(Four** out) {
  *out = nullptr;
  auto f = std::make_unique<Four>();
  if (int rc = f->a.alloc(64)) return rc;
  if (int rc = f->b.alloc(1024)) return rc;
  if (int rc = f->c.alloc(128)) return rc;
  if (int rc = f->d.alloc(128)) return rc;
  *out = f.release();
  return 0;
}

}  // namespace

TEST(Buffer, AllocOwnsAndFreesOnce) {
  Clean clean;
  {
    Buf<double> b;
    EXPECT_TRUE(b.empty() && !b && b.get() == nullptr && b.capacity() == 0);
    EXPECT_EQ(b.alloc(10), 0);
    EXPECT_TRUE(!b.empty() && b && b.get() != nullptr);
    EXPECT_EQ(b.capacity(), 10u);
    b.get()[9] = 1.0;   // (10 doubles, not 10 bytes: ASan sees the difference)
    EXPECT_EQ(heap.live.size(), 1u);
    EXPECT_EQ(b.reset(), 0);
    EXPECT_TRUE(b.empty() && b.capacity() == 0);
    EXPECT_EQ(b.reset(), 0);   // (nothing to free: no call)
    EXPECT_EQ(heap.calls, std::string("AF"));
    Buf<void> bytes;
    EXPECT_EQ(bytes.alloc(7), 0);
    EXPECT_EQ(bytes.capacity(), 7u);
    static_cast<char*>(bytes.get())[6] = 1;
  }
  EXPECT_EQ(heap.calls, std::string("AFAF"));
}

TEST(Buffer, FailedAllocLeavesItEmpty) {
  Clean clean;
  Buf<int> b;
  heap.fresh(1);
  EXPECT_EQ(b.alloc(100), 2);   // (the policy's status, as it is)
  EXPECT_TRUE(b.empty() && b.capacity() == 0);
  EXPECT_EQ(b.alloc(100), 0);
  EXPECT_EQ(b.capacity(), 100u);
}

// alloc is meant for an empty buffer, but one that still holds a block gives it up rather than leak it
TEST(Buffer, AllocOnAHeldBufferFreesTheOldBlockFirst) {
  Clean clean;
  Buf<int> b;
  EXPECT_EQ(b.alloc(100), 0);
  int* const old = b.get();
  heap.fresh();
  EXPECT_EQ(b.alloc(10), 0);   // (smaller: alloc gives exactly n, unlike grow)
  EXPECT_EQ(heap.calls, std::string("FA"));
  EXPECT_TRUE(heap.live.count(old) == 0 && heap.live.size() == 1 && b.capacity() == 10);
  heap.fresh(1);
  EXPECT_EQ(b.alloc(20), 2);
  EXPECT_EQ(heap.calls, std::string("FA"));
  EXPECT_TRUE(b.empty() && b.capacity() == 0 && heap.live.empty());
}

TEST(Buffer, MoveTransfersOwnership) {
  Clean clean;
  Buf<int> a;
  EXPECT_EQ(a.alloc(8), 0);
  int* const pa = a.get();
  Buf<int> b(std::move(a));
  EXPECT_TRUE(a.empty() && a.capacity() == 0);
  EXPECT_TRUE(b.get() == pa && b.capacity() == 8);
  Buf<int> c;
  EXPECT_EQ(c.alloc(4), 0);
  int* const pc = c.get();
  heap.fresh();
  c = std::move(b);   // frees c's old block, takes b's
  EXPECT_EQ(heap.calls, std::string("F"));
  EXPECT_TRUE(heap.live.count(pc) == 0 && heap.live.count(pa) == 1);
  EXPECT_TRUE(b.empty() && c.get() == pa && c.capacity() == 8);
  Buf<int>& same = c;
  c = std::move(same);   // (self-assignment keeps the block)
  EXPECT_TRUE(c.get() == pa && heap.live.size() == 1);
}

TEST(Buffer, GrowOnlyWhenTheRequestDoesNotFit) {
  Clean clean;
  Buf<float> b;
  EXPECT_EQ(b.grow(0), 0);
  EXPECT_EQ(heap.calls, std::string(""));
  EXPECT_EQ(b.grow(100), 0);   // empty: nothing to free
  EXPECT_EQ(heap.calls, std::string("A"));
  float* const p = b.get();
  heap.fresh();
  EXPECT_EQ(b.grow(100), 0);
  EXPECT_EQ(b.grow(1), 0);
  EXPECT_TRUE(heap.calls.empty() && b.get() == p && b.capacity() == 100);
  EXPECT_EQ(b.grow(101), 0);   // free FIRST, then allocate
  EXPECT_EQ(heap.calls, std::string("FA"));
  EXPECT_EQ(b.capacity(), 101u);
  EXPECT_EQ(heap.live.size(), 1u);
}

// ensure_event_classes: after a failed growth the capacity must not say "large enough" over a null pointer
TEST(Buffer, FailedGrowLeavesItEmptyAndASmallerGrowAllocatesAgain) {
  Clean clean;
  Buf<int> b;
  EXPECT_EQ(b.grow(100), 0);
  heap.fresh(1);
  EXPECT_EQ(b.grow(1000), 2);
  EXPECT_EQ(heap.calls, std::string("FA"));
  EXPECT_TRUE(b.empty() && b.capacity() == 0 && heap.live.empty());
  heap.fresh();
  EXPECT_EQ(b.grow(50), 0);   // (50 fitted the old capacity; the buffer no longer claims it)
  EXPECT_EQ(heap.calls, std::string("A"));
  EXPECT_TRUE(b.get() != nullptr && b.capacity() == 50);
  b.get()[49] = 1;
}

// sxmc_hist::retired: an outgrown block other descriptors may still point at is kept by a holder, not freed
TEST(Buffer, RetiredBlockIsFreedByItsHolder) {
  Clean clean;
  {
    std::vector<Buf<int>> retired;
    {
      Buf<int> b;
      EXPECT_EQ(b.alloc(10), 0);
      int* const old = b.get();
      heap.fresh();
      retired.push_back(std::move(b));
      EXPECT_EQ(b.alloc(20), 0);
      EXPECT_EQ(heap.calls, std::string("A"));   // no free: the old block lives on
      EXPECT_TRUE(heap.live.count(old) == 1 && retired.back().get() == old && b.get() != old);
      for (int i = 0; i < 3; i++) {   // (the holder may move its blocks about)
        Buf<int> next;
        EXPECT_EQ(next.alloc(4), 0);
        retired.push_back(std::move(next));
      }
      EXPECT_EQ(heap.live.count(old), 1u);
      heap.fresh();
    }
    EXPECT_EQ(heap.calls, std::string("F"));   // b's own block only
    EXPECT_EQ(heap.live.size(), 4u);
  }
  EXPECT_EQ(heap.calls, std::string("FFFFF"));
}

TEST(Buffer, CreationThatFailsAnywhereLeavesNothing) {
  Clean clean;
  for (int k = 0; k <= 4; k++) {
    heap.fresh(k);
    Four* f = reinterpret_cast<Four*>(1);
    const int rc = create_four(&f);
    EXPECT_EQ(rc, k ? 2 : 0);
    EXPECT_TRUE((f == nullptr) == (k != 0));
    EXPECT_EQ(heap.live.size(), k ? 0u : 4u);
    delete f;
    EXPECT_EQ(heap.live.size(), 0u);
  }
}

TEST(Buffer, GrowthThatFailsAnywhereLeaksNothingAndCanBeRepeated) {
  Clean clean;
  for (int k = 0; k <= 4; k++) {
    for (int round = 0; round < 2; round++) {   // on an empty object, and on one that holds smaller buffers
      Four f;
      if (round) EXPECT_EQ(f.fill(10), 0);
      heap.fresh(k);
      EXPECT_EQ(f.fill(100), k ? 2 : 0);
      EXPECT_EQ(heap.live.size(), f.owned());   // never a live block beyond what the object reports owning
      // (buffers before the k-th are new, the k-th is empty, those after it are as they were)
      EXPECT_EQ(f.owned(), !k ? 4u : round ? 3u : (size_t)(k - 1));
      heap.fresh();
      EXPECT_EQ(f.fill(100), 0);   // the same call again
      EXPECT_TRUE(f.owned() == 4 && heap.live.size() == 4);
      EXPECT_TRUE(f.a.capacity() == 100 && f.b.capacity() == 200 && f.c.capacity() == 125 && f.d.capacity() == 1600);
      heap.fresh(k);
      EXPECT_EQ(f.fill(50), 0);    // fits: no call, so nothing to fail
      EXPECT_TRUE(heap.calls.empty());
      EXPECT_EQ(f.fill(1000), k ? 2 : 0);
      EXPECT_EQ(heap.live.size(), f.owned());
      EXPECT_EQ(f.owned(), k ? 3u : 4u);
    }
    EXPECT_EQ(heap.live.size(), 0u);
  }
}

int main(int argc, char** argv) { return mini::run_all(argc > 1 ? argv[1] : nullptr); }
