// Host test of mpassit_amd/csrc/store_cache.h (tests/test_store_cache.py builds and runs it): the key, the cache and the worker's queue
// that every RegridStore passes through, with a stub handle and a build the test holds at a latch.  No GPU, nothing loaded into Python.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <vector>

#include "../../mpassit_amd/csrc/store_cache.h"

#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

// ---- the stub handle: every one made is counted, every one freed is remembered in order -----------------------------------------
struct Stub {
  int refcount = 1;
  bool cached = false;
  uint64_t parked_at = 0;
  StoreKey key;
  int id;
};
static std::mutex g_mu;
static int g_made = 0;
static std::vector<int> g_freed;
static Stub *make_stub(int refcount = 0) {
  std::lock_guard<std::mutex> lk(g_mu);
  Stub *h = new Stub();
  h->refcount = refcount;
  h->id = g_made++;
  return h;
}
static void free_stub(Stub *h) {
  std::lock_guard<std::mutex> lk(g_mu);
  CHECK(std::find(g_freed.begin(), g_freed.end(), h->id) == g_freed.end());   // exactly once
  g_freed.push_back(h->id);
  delete h;
}
static bool was_freed(int id) {
  std::lock_guard<std::mutex> lk(g_mu);
  return std::find(g_freed.begin(), g_freed.end(), id) != g_freed.end();
}
typedef StoreCache<Stub> Cache;

static char g_obj[64];   // addresses that stand for meshes and grids
static const void *A = &g_obj[0], *B = &g_obj[1], *G = &g_obj[2];
static StoreKey some_key(int i) { return StoreKey::grid_to_mesh(G, 0, &g_obj[8 + i], 0, MPG_REGRIDMETHOD_NEAREST_STOD, 10); }

// ---- keys ------------------------------------------------------------------------------------------------------------------------
// The key as the library packed it before StoreKey: (source, location code, destination, location, method + options + kind bits).
typedef std::tuple<const void *, int, const void *, int, int> OldKey;
struct Knobs { int linetype, fan_origin, tol_exp; };
struct Pair { OldKey was; StoreKey is; };

static void all_keys(const Knobs &kn, std::vector<Pair> &out) {
  const int BIL = MPG_REGRIDMETHOD_BILINEAR, CON = MPG_REGRIDMETHOD_CONSERVE, NODE = MPG_MESHLOC_NODE, ELEM = MPG_MESHLOC_ELEMENT;
  const int TO_MESH = 1 << 20, MESH_MESH = 1 << 21, PERIODIC = 1 << 22;
  const void *meshes[2] = {A, B};
  for (const void *m : meshes) {
    // mpg_regrid_store / _begin: node-located sources bilinear only, conservative onto CENTER only
    for (int loc = 0; loc <= 1; ++loc)
      for (int st = 0; st <= 2; ++st)
        for (int method = 0; method <= 2; ++method) {
          if (loc == NODE && method != BIL) continue;
          if (method == CON && st != MPG_STAGGERLOC_CENTER) continue;
          out.push_back({OldKey(m, loc, G, st, method + (method == BIL ? 16 * kn.linetype : 0) + (method == BIL && loc == NODE ? 256 * (kn.fan_origin + 16) : 0)),
                         StoreKey::mesh_to_grid(m, loc, G, st, method, kn.linetype, kn.fan_origin)});
        }
    // mpg_regrid_store_to_mesh: every stagger, the three mesh locations, bilinear and nearest
    for (int st = 0; st <= 3; ++st)
      for (int loc = 0; loc <= 2; ++loc)
        for (int method = 0; method <= 2; ++method) {
          if (method == CON) continue;
          out.push_back({OldKey(G, 200 + st, m, loc, method + (method == BIL ? 256 * kn.tol_exp : 0) + TO_MESH),
                         StoreKey::grid_to_mesh(G, st, m, loc, method, kn.tol_exp)});
        }
    for (int loc = 0; loc <= 1; ++loc)
      for (int pole = 0; pole <= 1; ++pole)
        out.push_back({OldKey(G, 200 + MPG_STAGGERLOC_CENTER, m, loc, BIL + 256 * kn.tol_exp + 65536 * pole + TO_MESH + PERIODIC),
                       StoreKey::periodic_to_mesh(G, m, loc, pole, kn.tol_exp)});
    for (int norm = 0; norm <= 1; ++norm)
      out.push_back({OldKey(G, 200 + MPG_STAGGERLOC_CENTER, m, ELEM, CON + 256 * norm + TO_MESH), StoreKey::conserve_to_mesh(G, m, norm)});
    for (const void *d : meshes) {
      // mpg_regrid_store_mesh: sources are the cells; bilinear and nearest
      for (int dloc = 0; dloc <= 1; ++dloc)
        for (int method = 0; method <= 2; ++method) {
          if (method == CON) continue;
          out.push_back({OldKey(m, ELEM, d, dloc, method + (method == BIL ? 16 * kn.linetype : 0) + MESH_MESH),
                         StoreKey::mesh_to_mesh(m, ELEM, d, dloc, method, kn.linetype)});
        }
      for (int norm = 0; norm <= 1; ++norm)
        out.push_back({OldKey(m, ELEM, d, ELEM, CON + 256 * norm + MESH_MESH), StoreKey::conserve_mesh_to_mesh(m, d, norm)});
    }
  }
  // mpg_regrid_store_grid / _begin: bilinear CENTER -> EDGE1 / EDGE2
  for (int st = MPG_STAGGERLOC_EDGE1; st <= MPG_STAGGERLOC_EDGE2; ++st)
    out.push_back({OldKey(G, 100 + MPG_STAGGERLOC_CENTER, G, st, BIL + 256 * kn.tol_exp), StoreKey::grid_to_grid(G, MPG_STAGGERLOC_CENTER, st, BIL, kn.tol_exp)});
}

static void test_keys() {
  std::vector<Pair> all;
  for (int lt = 0; lt <= 1; ++lt)
    for (int fo = -8; fo <= 15; ++fo)
      for (int tol : {10, 6}) all_keys(Knobs{lt, fo, tol}, all);
  // was(i) == was(j) <=> is(i) == is(j) over all pairs (i, j): each old key meets one new key only, and each new key one old key only
  std::map<OldKey, StoreKey> fwd;
  std::map<StoreKey, OldKey> back;
  for (const Pair &p : all) {
    auto f = fwd.emplace(p.was, p.is);
    CHECK(f.first->second == p.is);
    auto b = back.emplace(p.is, p.was);
    CHECK(b.first->second == p.was);
    CHECK(!(p.is < p.is));
  }
  CHECK(fwd.size() == back.size());
  // ... and literally, over the pairs of one knob setting against another (the full square is the two maps above)
  std::vector<Pair> k0, k1;
  all_keys(Knobs{0, 0, 10}, k0);
  all_keys(Knobs{1, -1, 6}, k1);
  for (const Pair &p : k0)
    for (const Pair &q : k1) {
      CHECK((p.was == q.was) == (p.is == q.is));
      CHECK((p.was < q.was || q.was < p.was) == (p.is < q.is || q.is < p.is));
    }
  const int BIL = MPG_REGRIDMETHOD_BILINEAR, NN = MPG_REGRIDMETHOD_NEAREST_STOD, CON = MPG_REGRIDMETHOD_CONSERVE;
  // nearest (and conservative) ignore the line type; bilinear does not
  CHECK(StoreKey::mesh_to_grid(A, 0, G, 0, NN, 0, 0) == StoreKey::mesh_to_grid(A, 0, G, 0, NN, 1, 0));
  CHECK(StoreKey::mesh_to_grid(A, 0, G, 0, CON, 0, 0) == StoreKey::mesh_to_grid(A, 0, G, 0, CON, 1, 0));
  CHECK(!(StoreKey::mesh_to_grid(A, 0, G, 0, BIL, 0, 0) == StoreKey::mesh_to_grid(A, 0, G, 0, BIL, 1, 0)));
  CHECK(StoreKey::mesh_to_mesh(A, 0, B, 0, NN, 0) == StoreKey::mesh_to_mesh(A, 0, B, 0, NN, 1));
  CHECK(!(StoreKey::mesh_to_mesh(A, 0, B, 0, BIL, 0) == StoreKey::mesh_to_mesh(A, 0, B, 0, BIL, 1)));
  // the fan origin enters node-located bilinear keys only
  CHECK(!(StoreKey::mesh_to_grid(A, 1, G, 0, BIL, 0, 0) == StoreKey::mesh_to_grid(A, 1, G, 0, BIL, 0, -1)));
  CHECK(StoreKey::mesh_to_grid(A, 0, G, 0, BIL, 0, 0) == StoreKey::mesh_to_grid(A, 0, G, 0, BIL, 0, -1));
  CHECK(StoreKey::mesh_to_grid(A, 0, G, 0, NN, 0, 0) == StoreKey::mesh_to_grid(A, 0, G, 0, NN, 0, -1));
  // the inside tolerance: Grid -> Grid, bilinear Grid -> Mesh and periodic keys
  CHECK(!(StoreKey::grid_to_grid(G, 0, 1, BIL, 10) == StoreKey::grid_to_grid(G, 0, 1, BIL, 6)));
  CHECK(!(StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10) == StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 6)));
  CHECK(StoreKey::grid_to_mesh(G, 0, A, 0, NN, 10) == StoreKey::grid_to_mesh(G, 0, A, 0, NN, 6));
  CHECK(!(StoreKey::periodic_to_mesh(G, A, 0, 0, 10) == StoreKey::periodic_to_mesh(G, A, 0, 0, 6)));
  CHECK(!(StoreKey::periodic_to_mesh(G, A, 0, 0, 10) == StoreKey::periodic_to_mesh(G, A, 0, 1, 10)));
  // whose source is a mesh
  CHECK(StoreKey::mesh_to_grid(A, 1, G, 0, BIL, 0, 0).source_is_mesh() && StoreKey::mesh_to_grid(A, 1, G, 0, BIL, 0, 0).source_mesh_loc() == 1);
  CHECK(StoreKey::mesh_to_mesh(A, 0, B, 1, BIL, 0).source_is_mesh() && StoreKey::mesh_to_mesh(A, 0, B, 1, BIL, 0).source_mesh_loc() == 0);
  CHECK(StoreKey::conserve_mesh_to_mesh(A, B, 0).source_is_mesh());
  CHECK(!StoreKey::grid_to_grid(G, 0, 1, BIL, 10).source_is_mesh());
  CHECK(!StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10).source_is_mesh());
  CHECK(!StoreKey::periodic_to_mesh(G, A, 0, 0, 10).source_is_mesh());
  CHECK(!StoreKey::conserve_to_mesh(G, A, 0).source_is_mesh());
  CHECK(StoreKey::mesh_to_mesh(A, 0, B, 1, BIL, 0).source_is(A, 0) && !StoreKey::mesh_to_mesh(A, 0, B, 1, BIL, 0).source_is(B, 1));
  CHECK(!StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10).source_is(A, 0));
  CHECK(StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10).touches(A) && StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10).touches(G) &&
        !StoreKey::grid_to_mesh(G, 0, A, 0, BIL, 10).touches(B));
  printf("keys: %zu calls under 96 knob settings, %zu distinct keys, old and new equality agree\n", all.size(), fwd.size());
}

// ---- cache -----------------------------------------------------------------------------------------------------------------------
static void test_cache() {
  {   // insert-if-absent never replaces
    Cache c(free_stub, 8);
    Stub *h1 = make_stub(), *h2 = make_stub();
    const int id2 = h2->id;
    CHECK(c.insert_if_absent(some_key(0), h1) == nullptr);
    CHECK(h1->cached && h1->key == some_key(0));
    Stub *spare = c.insert_if_absent(some_key(0), h2);
    CHECK(spare == h2 && !h2->cached);
    c.free_unowned(spare);
    CHECK(was_freed(id2));
    Stub *got = c.find_ref(some_key(0));
    CHECK(got == h1 && h1->refcount == 1);
    CHECK(c.find_ref(some_key(1)) == nullptr && c.contains(some_key(0)) && !c.contains(some_key(1)));
    c.release(got);
    c.drop_parked();
    CHECK(!c.contains(some_key(0)));
  }
  for (int n : {9, 10, 12}) {   // more than 8 parked: the one released longest ago goes, whatever its key
    Cache c(free_stub, 8);
    std::vector<Stub *> h((size_t)n);
    std::vector<int> id((size_t)n), order;
    for (int i = 0; i < n; ++i) {
      h[(size_t)i] = make_stub();
      id[(size_t)i] = h[(size_t)i]->id;
      CHECK(c.insert_if_absent(some_key(i), h[(size_t)i]) == nullptr);
      CHECK(c.find_ref(some_key(i)) == h[(size_t)i]);
    }
    for (int i = 0; i < n; ++i) order.push_back((i * 5 + 3) % n);   // a release order that is not the key order (5 is coprime to 9, 12; n = 10: below)
    if (n == 10) for (int i = 0; i < n; ++i) order[(size_t)i] = (i * 7 + 3) % n;
    size_t f0;
    {
      std::lock_guard<std::mutex> lk(g_mu);
      f0 = g_freed.size();
    }
    for (int i = 0; i < n; ++i) {
      c.release(h[(size_t)order[(size_t)i]]);
      std::lock_guard<std::mutex> lk(g_mu);
      CHECK(g_freed.size() - f0 == (size_t)std::max(0, i + 1 - 8));
    }
    {
      std::lock_guard<std::mutex> lk(g_mu);
      for (int i = 0; i < n - 8; ++i) CHECK(g_freed[f0 + (size_t)i] == id[(size_t)order[(size_t)i]]);   // in release order
    }
    for (int i = n - 8; i < n; ++i) CHECK(c.contains(some_key(order[(size_t)i])));
    c.drop_parked();
  }
  {   // a held entry is never evicted, however long ago it went in
    Cache c(free_stub, 8);
    Stub *held = make_stub();
    const int held_id = held->id;
    CHECK(!c.insert_if_absent(some_key(20), held) && c.find_ref(some_key(20)) == held);
    for (int i = 0; i < 11; ++i) {
      Stub *h = make_stub();
      CHECK(!c.insert_if_absent(some_key(i), h) && c.find_ref(some_key(i)) == h);
      c.release(h);
    }
    CHECK(!was_freed(held_id) && c.contains(some_key(20)) && held->cached);
    CHECK(!c.contains(some_key(0)) && !c.contains(some_key(2)) && c.contains(some_key(3)));
    c.drop_parked();   // parked ones only
    CHECK(!was_freed(held_id) && c.contains(some_key(20)));
    c.release(held);
    c.drop_parked();
    CHECK(was_freed(held_id));
  }
  {   // purge by object, in the source and in the destination place; drop_parked by object
    Cache c(free_stub, 8);
    const StoreKey src_a = StoreKey::mesh_to_grid(A, 0, G, 0, 0, 0, 0), dst_a = StoreKey::grid_to_mesh(G, 0, A, 0, 0, 10);
    const StoreKey src_a2 = StoreKey::mesh_to_mesh(A, 0, B, 0, 0, 0), dst_a2 = StoreKey::mesh_to_mesh(B, 0, A, 1, 0, 0);
    const StoreKey other = StoreKey::mesh_to_mesh(B, 0, B, 0, 0, 0);
    Stub *p1 = make_stub(), *p2 = make_stub(), *k1 = make_stub(), *k2 = make_stub(), *o = make_stub();
    const int ids[5] = {p1->id, p2->id, k1->id, k2->id, o->id};
    CHECK(!c.insert_if_absent(src_a, p1) && !c.insert_if_absent(dst_a, p2) && !c.insert_if_absent(src_a2, k1) && !c.insert_if_absent(dst_a2, k2) &&
          !c.insert_if_absent(other, o));
    CHECK(c.find_ref(src_a2) == k1 && c.find_ref(dst_a2) == k2);
    c.purge(A);
    CHECK(was_freed(ids[0]) && was_freed(ids[1]) && !was_freed(ids[2]) && !was_freed(ids[3]) && !was_freed(ids[4]));
    CHECK(!k1->cached && !k2->cached && !c.contains(src_a) && !c.contains(dst_a) && !c.contains(src_a2) && !c.contains(dst_a2) && c.contains(other));
    c.release(k1);   // un-cached: the last release frees
    c.release(k2);
    CHECK(was_freed(ids[2]) && was_freed(ids[3]));
    c.drop_parked(A);
    CHECK(c.contains(other));
    c.drop_parked(B);
    CHECK(!c.contains(other) && was_freed(ids[4]));
  }
  {   // detach, then release: frees the handle and leaves another handle's entry under the same key alone
    Cache c(free_stub, 8);
    Stub *h1 = make_stub(), *h2 = make_stub();
    const int id1 = h1->id, id2 = h2->id;
    CHECK(!c.insert_if_absent(some_key(0), h1) && c.find_ref(some_key(0)) == h1);
    c.detach(h1);
    CHECK(!h1->cached && !c.contains(some_key(0)));
    CHECK(!c.insert_if_absent(some_key(0), h2));
    c.detach(h1);   // again: nothing
    c.release(h1);
    CHECK(was_freed(id1) && !was_freed(id2) && c.contains(some_key(0)) && c.find_ref(some_key(0)) == h2);
    c.release(h2);
    // the visit: busy while it lasts, every entry seen
    CHECK(!c.busy());
    const int seen = c.with_entries([&](const Cache::Map &m) {
      CHECK(c.busy());
      return (int)m.size();
    });
    CHECK(seen == 1 && !c.busy());
    c.drop_parked();
    CHECK(was_freed(id2));
  }
  printf("cache: ok\n");
}

// ---- queue -----------------------------------------------------------------------------------------------------------------------
struct Latch {
  std::mutex m;
  std::condition_variable cv;
  bool held = false;
  int arrived = 0;
  void hold() {
    std::lock_guard<std::mutex> lk(m);
    held = true;
  }
  void open() {
    {
      std::lock_guard<std::mutex> lk(m);
      held = false;
    }
    cv.notify_all();
  }
  void pass() {   // whoever comes by is counted and waits while the latch is held
    std::unique_lock<std::mutex> lk(m);
    ++arrived;
    cv.notify_all();
    cv.wait(lk, [&] { return !held; });
  }
  void wait_arrived(int n) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return arrived >= n; });
  }
};
struct Work { int filled = 0; };
typedef StoreQueue<Stub, Work> Queue;
struct Rig {
  Cache cache{free_stub, 8};
  Latch build_latch;
  std::atomic<int> builds{0}, fills{0};
  bool fail = false;
  char stream_tag = 0;
  Queue *q;
  Rig() {
    q = new Queue(cache, [this](Queue::Job &job, void *stream) {
      CHECK(stream == &stream_tag && job.work.filled == 1 && !job.handle);
      ++builds;
      build_latch.pass();
      if (fail) {
        job.err = "boom in key of dst_loc " + std::to_string(job.key.dst_loc);
        return 7;
      }
      job.handle = make_stub();
      return 0;
    });
  }
  int start(int bind_rc = 0) {
    return q->start([this](void **s) { *s = &stream_tag; return 0; },
                    [bind_rc](std::string &err) { if (bind_rc) err = "no device"; return bind_rc; });
  }
  std::function<void(Queue::Job &)> fill() {
    return [this](Queue::Job &job) { job.work.filled++; ++fills; };
  }
  ~Rig() {
    (void)q->stop();
    cache.drop_parked();
    delete q;   // the worker has been joined: nobody waits on its condition variable
  }
};

static void test_queue() {
  {   // 8 threads, one key, the build held: one build, one handle, eight references
    Rig r;
    CHECK(r.start() == 0 && r.start() == 0);
    r.build_latch.hold();
    std::atomic<int> entered{0};
    Stub *got[8] = {};
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
      th.emplace_back([&, t] {
        ++entered;
        std::string err;
        CHECK(r.q->get(some_key(0), &got[t], r.fill(), &err) == 0);
      });
    r.build_latch.wait_arrived(1);
    while (entered < 8) std::this_thread::yield();
    for (int i = 0; i < 2000; ++i) std::this_thread::yield();   // most of them wait on the job by now; the result must not depend on it
    r.build_latch.open();
    for (auto &t : th) t.join();
    CHECK(r.builds == 1 && r.fills == 1);
    for (int t = 0; t < 8; ++t) CHECK(got[t] && got[t] == got[0]);
    CHECK(got[0]->refcount == 8 && got[0]->cached);
    for (int t = 0; t < 8; ++t) r.cache.release(got[t]);
  }
  {   // ADVICE finding 2: a finished job of the key is inserted while a caller sits between its lookup and its enqueue.  In this
      // queue that place is inside get's lock and the worker publishes under the same lock, so only the test itself can insert there: it does
      // what the worker of the old code did (insert into the cache, nothing else) while the caller is stopped in fill().  The caller's own job
      // then finishes second: the entry stays, the second handle is freed, nobody is left with a handle the cache does not know.
    Rig r;
    CHECK(r.start() == 0);
    Latch in_fill;
    in_fill.hold();
    Stub *first = make_stub();
    const int first_id = first->id;
    Stub *got = nullptr;
    std::thread caller([&] {
      std::string err;
      CHECK(r.q->get(some_key(1), &got, [&](Queue::Job &job) {
        job.work.filled++;
        in_fill.pass();
      }, &err) == 0);
    });
    in_fill.wait_arrived(1);
    std::atomic<bool> second_done{false};
    Stub *got2 = nullptr;
    std::thread second([&] {   // a second caller cannot slip in between either: it waits for the lock, then finds the entry
      std::string err;
      CHECK(r.q->get(some_key(1), &got2, r.fill(), &err) == 0);
      second_done = true;
    });
    for (int i = 0; i < 2000; ++i) std::this_thread::yield();
    CHECK(!second_done && r.builds == 0);
    CHECK(r.cache.insert_if_absent(some_key(1), first) == nullptr);
    in_fill.open();
    caller.join();
    second.join();
    CHECK(r.builds == 1 && r.fills == 0);
    CHECK(got == first && got2 == first && first->refcount == 2 && first->cached);
    {
      std::lock_guard<std::mutex> lk(g_mu);
      CHECK(g_freed.size() == (size_t)g_made - 1);   // every handle but `first` is gone: the spare of the second build among them
    }
    r.cache.release(got);
    r.cache.release(got2);
    r.cache.drop_parked();
    CHECK(was_freed(first_id));
  }
  {   // _begin twice, then a collect: one build; a collect after the build: from the cache
    Rig r;
    CHECK(r.start() == 0);
    r.build_latch.hold();
    std::string err;
    CHECK(r.q->get(some_key(2), nullptr, r.fill(), &err) == 0);
    CHECK(r.q->get(some_key(2), nullptr, r.fill(), &err) == 0);
    r.build_latch.open();
    Stub *a = nullptr, *b = nullptr;
    CHECK(r.q->get(some_key(2), &a, r.fill(), &err) == 0 && a);
    r.q->drain();
    CHECK(r.q->get(some_key(2), nullptr, r.fill(), &err) == 0);
    CHECK(r.q->get(some_key(2), &b, r.fill(), &err) == 0 && b == a && a->refcount == 2);
    CHECK(r.builds == 1 && r.fills == 1);
    r.cache.release(a);
    r.cache.release(b);
  }
  {   // a build that fails: every waiter gets its rc and its text, nothing is cached, the next call builds again
    Rig r;
    CHECK(r.start() == 0);
    r.fail = true;
    r.build_latch.hold();
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
      th.emplace_back([&] {
        std::string err;
        Stub *h = (Stub *)&g_obj[40];
        CHECK(r.q->get(some_key(3), &h, r.fill(), &err) == 7);
        CHECK(h == nullptr && err == "boom in key of dst_loc 0");
      });
    r.build_latch.wait_arrived(1);
    r.build_latch.open();
    for (auto &t : th) t.join();
    r.q->drain();
    CHECK(!r.cache.contains(some_key(3)));
    r.fail = false;
    Stub *h = nullptr;
    std::string err;
    CHECK(r.q->get(some_key(3), &h, r.fill(), &err) == 0 && h && h->refcount == 1);
    r.cache.release(h);
  }
  {   // stop with a queue that is not empty: every job runs first
    Rig r;
    CHECK(r.start() == 0);
    r.build_latch.hold();
    std::string err;
    for (int i = 0; i < 3; ++i) CHECK(r.q->get(some_key(4 + i), nullptr, r.fill(), &err) == 0);
    r.build_latch.wait_arrived(1);
    void *stream = nullptr;
    std::thread stopper([&] { stream = r.q->stop(); });
    for (int i = 0; i < 2000; ++i) std::this_thread::yield();
    CHECK(r.builds == 1);
    r.build_latch.open();
    stopper.join();
    CHECK(stream == &r.stream_tag && r.builds == 3);
    for (int i = 0; i < 3; ++i) CHECK(r.cache.contains(some_key(4 + i)));
    CHECK(r.q->stop() == nullptr);
    CHECK(r.start() == 0);   // and it starts again (mpg_finalize, then mpg_init)
    Stub *h = nullptr;
    CHECK(r.q->get(some_key(7), &h, r.fill(), &err) == 0 && h && r.builds == 4);
    r.cache.release(h);
  }
  {   // a worker that cannot bind its device serves the queue with the error
    Rig r;
    CHECK(r.start(5) == 0);
    for (int i = 0; i < 2; ++i) {
      Stub *h = nullptr;
      std::string err;
      CHECK(r.q->get(some_key(i), &h, r.fill(), &err) == 5 && !h && err == "no device");
    }
    CHECK(r.builds == 0 && !r.cache.contains(some_key(0)));
  }
  printf("queue: ok\n");
}

int main() {
  test_keys();
  test_cache();
  test_queue();
  std::lock_guard<std::mutex> lk(g_mu);
  CHECK(g_made > 0 && (size_t)g_made == g_freed.size());
  printf("handles made %d freed %zu\nok\n", g_made, g_freed.size());
  return 0;
}
