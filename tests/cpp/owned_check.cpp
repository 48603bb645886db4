// CPU check of tbv_slam_public_amd/csrc/owned.hpp: the unique_ptr + stateless deleter shape that owns the library's long-lived
// device memory, pinned memory, events, streams and graphs, bound here to counting stand-ins for the HIP free functions (no
// HIP runtime).  The stand-ins keep the set of live blocks, so a double free or a free of a foreign pointer fails the check,
// and the blocks are real heap blocks, so a build with -fsanitize=address reports a leak or a use after free as well.
// The cases are the moves the library makes: a buffer replaced and reset (workspace growth), a slab that travels between a
// scan and the context's free list, an early return between an allocation and its hand-over (the descriptor database's growth,
// the *_create functions), a handle struct whose stream must outlive the buffers and events used on it.
// Prints "<allocations> <frees>" and returns 0, or the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../tbv_slam_public_amd/csrc/owned.hpp"

static int g_allocs = 0, g_frees = 0, g_bad = 0;
static std::set<void*> g_live;
static std::vector<void*> g_free_order;

static void* fake_malloc(size_t bytes) {
  void* p = std::malloc(bytes ? bytes : 256);
  g_allocs++;
  g_live.insert(p);
  return p;
}
// the signature of hipFree / hipHostFree: takes void*, returns a status the deleter ignores
static int fake_free(void* p) {
  if (!g_live.erase(p)) { g_bad++; return 1; }   // a double free, or a pointer nothing allocated
  g_frees++;
  g_free_order.push_back(p);
  std::free(p);
  return 0;
}
// the signature of hipEventDestroy / hipStreamDestroy: an opaque handle type, a pointer to an incomplete struct
struct fake_handle_s;
typedef fake_handle_s* fake_handle_t;
static int fake_handle_destroy(fake_handle_t h) { return fake_free((void*)h); }

template <class T> using Buf = Owned<T, fake_free>;
template <class T> using HostBuf = Owned<T[], fake_free>;
using Handle = Owned<std::remove_pointer_t<fake_handle_t>, fake_handle_destroy>;
template <class T> static Buf<T> buf_alloc(size_t bytes, bool fail = false) { return Buf<T>(fail ? nullptr : (T*)fake_malloc(bytes)); }
static Handle make_handle(bool fail = false) { return Handle(fail ? nullptr : (fake_handle_t)fake_malloc(8)); }

static_assert(sizeof(Buf<char>) == sizeof(char*), "a stateless deleter adds nothing to the pointer");
static_assert(!std::is_copy_constructible<Buf<char>>::value, "one owner at a time");

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

// cfear_scan / cfear_ctx::free_slabs
struct Slab { Buf<void> p; int cap; };
struct Scan { Buf<void> slab; int cap = 0; };
struct Ctx { std::vector<Slab> free_slabs; };

static Scan* scan_alloc(Ctx& ctx, int cap) {
  Buf<void> slab;
  for (size_t i = 0; i < ctx.free_slabs.size(); i++)
    if (ctx.free_slabs[i].cap >= cap) {
      slab = std::move(ctx.free_slabs[i].p);
      cap = ctx.free_slabs[i].cap;
      ctx.free_slabs.erase(ctx.free_slabs.begin() + (long)i);
      break;
    }
  if (!slab && !(slab = buf_alloc<void>((size_t)cap))) return nullptr;
  Scan* s = new Scan();
  s->slab = std::move(slab);
  s->cap = cap;
  return s;
}
static void scan_destroy(Ctx& ctx, Scan* s) {
  ctx.free_slabs.push_back(Slab{std::move(s->slab), s->cap});
  delete s;
}

// sc_manager_commit's growth: the new block replaces the database only once the copy into it has succeeded
struct Db { Buf<double> d_db; int cap = 0; };
static int db_grow(Db& db, bool fail_alloc, bool fail_copy) {
  const int ncap = db.cap ? db.cap * 2 : 4;
  Buf<double> nd = buf_alloc<double>((size_t)ncap * sizeof(double), fail_alloc);
  if (!nd) return 1;
  if (fail_copy) return 2;               // the early return: nd is freed here, the database is untouched
  db.d_db = std::move(nd);               // frees the old block
  db.cap = ncap;
  return 0;
}

// a handle struct and its *_create: the object sits in an owner whose deleter is the handle's own destroy function
struct Pipe {
  Handle stream;                         // declared first: destroyed last
  Buf<char> d_send;
  HostBuf<int> h_recv;
  Handle done;
};
static int g_pipe_destroyed = 0;
static int pipe_destroy(Pipe* p) {
  if (!p) return 0;
  g_pipe_destroyed++;
  delete p;
  return 0;
}
static int pipe_create(int fail_at, Pipe** out) {
  *out = nullptr;
  std::unique_ptr<Pipe, FreeWith<pipe_destroy>> p(new Pipe());
  bool ok = bool(p->stream = make_handle(fail_at == 0));
  ok = ok && (p->d_send = buf_alloc<char>(64, fail_at == 1));
  ok = ok && (p->h_recv = HostBuf<int>(fail_at == 2 ? nullptr : (int*)fake_malloc(16 * sizeof(int))));
  ok = ok && (p->done = make_handle(fail_at == 3));
  if (!ok) return 1;                     // the early return: whatever was made so far goes with the object, once
  *out = p.release();
  return 0;
}

int main() {
  // move out of an owner and reset it
  {
    Buf<char> a = buf_alloc<char>(100);
    char* raw = a.get();
    CHECK(a && g_allocs == 1 && g_frees == 0);
    Buf<char> b = std::move(a);
    CHECK(!a && b.get() == raw && g_frees == 0);
    b.reset();
    CHECK(!b && g_frees == 1);
    b.reset();                                               // an empty owner frees nothing
    CHECK(g_frees == 1);
    b = buf_alloc<char>(0);                                  // the growth of a workspace: reset, then a larger block
    b = buf_alloc<char>(200);
    CHECK(g_allocs == 3 && g_frees == 2);
    Buf<char> none = buf_alloc<char>(1, true);               // a failed allocation is an empty owner
    CHECK(!none && g_allocs == 3);
  }
  CHECK(g_allocs == 3 && g_frees == 3 && g_live.empty());

  // a slab moves from a scan into the free list and back
  {
    Ctx ctx;
    Scan* s = scan_alloc(ctx, 100);
    CHECK(s && s->slab);
    void* raw = s->slab.get();
    scan_destroy(ctx, s);
    CHECK(ctx.free_slabs.size() == 1 && ctx.free_slabs[0].p.get() == raw && g_frees == 3);
    Scan* t = scan_alloc(ctx, 50);                           // the recycled slab, not a new one
    CHECK(t && t->slab.get() == raw && t->cap == 100 && ctx.free_slabs.empty() && g_allocs == 4);
    Scan* u = scan_alloc(ctx, 50);
    CHECK(u && u->slab.get() != raw && g_allocs == 5);
    scan_destroy(ctx, u);
    scan_destroy(ctx, t);
    CHECK(ctx.free_slabs.size() == 2 && g_frees == 3);
  }                                                          // the context goes: both slabs with it
  CHECK(g_allocs == 5 && g_frees == 5 && g_live.empty());

  // an early return between an allocation and its hand-over frees exactly once
  {
    Db db;
    CHECK(db_grow(db, false, false) == 0 && db.cap == 4 && g_allocs == 6 && g_frees == 5);
    double* raw = db.d_db.get();
    CHECK(db_grow(db, true, false) == 1 && db.d_db.get() == raw && db.cap == 4 && g_allocs == 6 && g_frees == 5);
    CHECK(db_grow(db, false, true) == 2 && db.d_db.get() == raw && db.cap == 4 && g_allocs == 7 && g_frees == 6);
    CHECK(db_grow(db, false, false) == 0 && db.d_db.get() != raw && db.cap == 8 && g_allocs == 8 && g_frees == 7);
  }
  CHECK(g_allocs == 8 && g_frees == 8 && g_live.empty());
  for (int fail_at = 0; fail_at < 4; fail_at++) {
    const int allocs = g_allocs, destroyed = g_pipe_destroyed;
    Pipe* p = nullptr;
    CHECK(pipe_create(fail_at, &p) == 1 && !p);
    CHECK(g_pipe_destroyed == destroyed + 1 && g_allocs == allocs + fail_at && g_frees == g_allocs && g_live.empty());
  }

  // a handle struct: the stream outlives the buffers and events used on it; pinned memory is indexed through its owner
  {
    Pipe* p = nullptr;
    CHECK(pipe_create(-1, &p) == 0 && p && g_live.size() == 4);
    for (int i = 0; i < 16; i++) p->h_recv[i] = i;
    CHECK(p->h_recv[15] == 15 && p->h_recv.get()[3] == 3);
    void* stream = (void*)p->stream.get();
    g_free_order.clear();
    pipe_destroy(p);
    CHECK(g_free_order.size() == 4 && g_free_order.back() == stream);
  }

  CHECK(g_bad == 0 && g_allocs == g_frees && g_live.empty());
  std::printf("%d %d\n", g_allocs, g_frees);
  return 0;
}
