// What every RegridStore passes through on the host: the key a handle is cached under, the cache of finished handles and the queue of
// the Store worker.  Plain C++17 without HIP: tests/c/store_cache_test.cpp runs the same text on the host with a stub handle.
//
// Locks.  StoreQueue::mu_ is taken first, StoreCache::mu_ inside it, never the other way round: the cache calls nothing of the queue,
// and its free callback and visitors call nothing of the cache (StoreCache::busy() is what an allocator asks first).  The worker
// publishes a finished handle -- insert into the cache, leave `pending` -- under the queue's lock, and StoreQueue::get looks the key
// up in the cache, then in `pending`, then queues it, under that same lock: a key is in one of the two places or is built once.
#pragma once
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>

#include "../../include/mpassit_amd.h"

enum StoreKind {
  STORE_MESH_TO_GRID = 0,
  STORE_GRID_TO_GRID,
  STORE_GRID_TO_MESH,
  STORE_PERIODIC_TO_MESH,
  STORE_CONSERVE_TO_MESH,
  STORE_MESH_TO_MESH,
  STORE_CONSERVE_MESH_TO_MESH,
  STORE_GRID_TO_OTHER_GRID,
  STORE_CONSERVE_GRID_TO_GRID,
  STORE_KIND_COUNT
};

// What a handle IS: two handles with equal keys hold the same weights.  The knobs in force (mpg_tune) enter a key exactly where the
// Store reads them and are zero elsewhere, so a nearest Store under either line type is one handle.  The named constructors are the
// only way the library makes a key.
struct StoreKey {   // an aggregate: the constructors below list the fields in this order
  StoreKind kind = STORE_MESH_TO_GRID;
  const void *src = nullptr;   // mesh or grid object, by address
  int src_loc = 0;             // MPG_MESHLOC_* of a mesh, MPG_STAGGERLOC_* of a grid
  const void *dst = nullptr;
  int dst_loc = 0;
  int method = 0;              // MPG_REGRIDMETHOD_*
  int linetype = 0;            // "bilinear_linetype": bilinear Stores FROM a mesh
  int fan_origin = 0;          // "node_fan_origin": bilinear Mesh -> Grid Stores of node-located sources
  int inside_tol_exp = 0;      // "grid_inside_tol_exp": bilinear Stores FROM a grid
  int pole_method = 0;         // MPG_POLEMETHOD_*: the periodic Store
  int norm_type = 0;           // MPG_NORM_*: the two conservative Stores onto a mesh and the conservative Grid -> Grid Store

  static StoreKey mesh_to_grid(const void *mesh, int meshloc, const void *grid, int stagger, int method, int linetype, int fan_origin) {
    const bool bil = method == MPG_REGRIDMETHOD_BILINEAR;
    return {STORE_MESH_TO_GRID, mesh, meshloc, grid, stagger, method, bil ? linetype : 0, bil && meshloc == MPG_MESHLOC_NODE ? fan_origin : 0};
  }
  static StoreKey grid_to_grid(const void *grid, int src_stagger, int dst_stagger, int method, int inside_tol_exp) {
    return {STORE_GRID_TO_GRID, grid, src_stagger, grid, dst_stagger, method, 0, 0, inside_tol_exp};
  }
  static StoreKey grid_to_mesh(const void *grid, int stagger, const void *mesh, int meshloc, int method, int inside_tol_exp) {
    return {STORE_GRID_TO_MESH, grid, stagger, mesh, meshloc, method, 0, 0, method == MPG_REGRIDMETHOD_BILINEAR ? inside_tol_exp : 0};
  }
  static StoreKey periodic_to_mesh(const void *grid, const void *mesh, int meshloc, int pole_method, int inside_tol_exp) {
    return {STORE_PERIODIC_TO_MESH, grid, MPG_STAGGERLOC_CENTER, mesh, meshloc, MPG_REGRIDMETHOD_BILINEAR, 0, 0, inside_tol_exp, pole_method};
  }
  static StoreKey conserve_to_mesh(const void *grid, const void *mesh, int norm_type) {
    return {STORE_CONSERVE_TO_MESH, grid, MPG_STAGGERLOC_CENTER, mesh, MPG_MESHLOC_ELEMENT, MPG_REGRIDMETHOD_CONSERVE, 0, 0, 0, 0, norm_type};
  }
  static StoreKey mesh_to_mesh(const void *src_mesh, int src_meshloc, const void *dst_mesh, int dst_meshloc, int method, int linetype) {
    return {STORE_MESH_TO_MESH, src_mesh, src_meshloc, dst_mesh, dst_meshloc, method, method == MPG_REGRIDMETHOD_BILINEAR ? linetype : 0};
  }
  static StoreKey conserve_mesh_to_mesh(const void *src_mesh, const void *dst_mesh, int norm_type) {
    return {STORE_CONSERVE_MESH_TO_MESH, src_mesh, MPG_MESHLOC_ELEMENT, dst_mesh, MPG_MESHLOC_ELEMENT, MPG_REGRIDMETHOD_CONSERVE, 0, 0, 0, 0, norm_type};
  }
  // between two grids (mpg_regrid_store_grid_to_grid; src == dst allowed): a kind of its own, so it never meets grid_to_grid's keys
  static StoreKey grid_to_other_grid(const void *src_grid, int src_stagger, const void *dst_grid, int dst_stagger, int method, int inside_tol_exp,
                                     int pole_method, bool src_periodic) {
    const bool bil = method == MPG_REGRIDMETHOD_BILINEAR;
    return {STORE_GRID_TO_OTHER_GRID, src_grid, src_stagger, dst_grid, dst_stagger, method, 0, 0, bil ? inside_tol_exp : 0, bil && src_periodic ? pole_method : 0};
  }
  static StoreKey conserve_grid_to_grid(const void *src_grid, const void *dst_grid, int norm_type) {
    return {STORE_CONSERVE_GRID_TO_GRID, src_grid, MPG_STAGGERLOC_CENTER, dst_grid, MPG_STAGGERLOC_CENTER, MPG_REGRIDMETHOD_CONSERVE, 0, 0, 0, 0, norm_type};
  }

  bool touches(const void *obj) const { return src == obj || dst == obj; }
  // The handle's sources are points of the mesh `src`: a source window on that mesh (mpg_mesh_set_source_window) re-indexes it.  A mesh
  // that is a handle's DESTINATION does not count: the sources of a Grid -> Mesh handle are grid points.
  bool source_is_mesh() const { return kind == STORE_MESH_TO_GRID || kind == STORE_MESH_TO_MESH || kind == STORE_CONSERVE_MESH_TO_MESH; }
  int source_mesh_loc() const { return src_loc; }
  bool source_is(const void *mesh, int meshloc) const { return source_is_mesh() && src == mesh && src_loc == meshloc; }

  // (source and its location first: the handles of one mesh and location are visited by destination, then by options)
  auto tied() const { return std::tie(src, src_loc, dst, dst_loc, kind, norm_type, pole_method, inside_tol_exp, fan_origin, linetype, method); }
  bool operator<(const StoreKey &o) const { return tied() < o.tied(); }
  bool operator==(const StoreKey &o) const { return tied() == o.tied(); }
};

// The finished handles by key.  H has `int refcount`, `bool cached`, `uint64_t parked_at` and `StoreKey key`; the cache writes the
// last three and counts references down, the holders count them up through find_ref.  An entry with refcount 0 is PARKED: released, or
// finished by a _begin and not collected yet.  Parked entries stay until their mesh or grid goes (purge), the library is finalized, an
// allocation fails (drop_parked) or more than max_parked of them wait: then the one released longest ago goes.
template <class H>
class StoreCache {
 public:
  typedef std::map<StoreKey, H *> Map;
  explicit StoreCache(std::function<void(H *)> free_handle, int max_parked) : free_(std::move(free_handle)), max_parked_(max_parked) {}

  H *find_ref(const StoreKey &key) {   // the entry with one more reference, or nullptr
    std::lock_guard<std::mutex> lk(mu_);
    auto it = map_.find(key);
    if (it == map_.end()) return nullptr;
    it->second->refcount++;
    return it->second;
  }
  bool contains(const StoreKey &key) {
    std::lock_guard<std::mutex> lk(mu_);
    return map_.count(key) != 0;
  }
  // `h` (refcount 0) parks under `key`.  An entry that is there already STAYS: -> `h`, for the caller to free; nullptr when h went in.
  H *insert_if_absent(const StoreKey &key, H *h) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!map_.emplace(key, h).second) return h;
    h->key = key;
    h->cached = true;
    h->parked_at = ++clock_;
    return nullptr;
  }
  void release(H *h) {   // one reference less; the last one parks a cached handle and frees any other
    std::lock_guard<std::mutex> lk(mu_);
    if (--h->refcount > 0) return;
    if (!h->cached) {
      free_(h);
      return;
    }
    h->parked_at = ++clock_;
    int nparked = 0;
    for (auto &kv : map_) nparked += kv.second->refcount == 0;
    for (; nparked > max_parked_; --nparked) {
      auto old = map_.end();
      for (auto it = map_.begin(); it != map_.end(); ++it)
        if (it->second->refcount == 0 && (old == map_.end() || it->second->parked_at < old->second->parked_at)) old = it;
      H *victim = old->second;
      map_.erase(old);
      free_(victim);
    }
  }
  void detach(H *h) {   // a handle about to be re-indexed in place no longer is what its key says; its holder frees it by releasing it
    std::lock_guard<std::mutex> lk(mu_);
    if (!h->cached) return;
    auto it = map_.find(h->key);
    if (it != map_.end() && it->second == h) map_.erase(it);
    h->cached = false;
  }
  void purge(const void *obj) {   // a mesh or grid goes: its parked handles with it, its held ones leave the cache (a recycled address must never hit)
    std::lock_guard<std::mutex> lk(mu_);
    erase_if([&](const StoreKey &k, H *) { return k.touches(obj); });
  }
  void drop_parked(const void *obj = nullptr) {   // the parked handles of obj, or all of them
    std::lock_guard<std::mutex> lk(mu_);
    erase_if([&](const StoreKey &k, H *h) { return h->refcount == 0 && (!obj || k.touches(obj)); });
  }
  // f(map) under the lock, for a caller that works on several entries (mpg_mesh_set_source_window's two passes).  busy() is true
  // meanwhile, on every thread: the entries must stay, so an allocator that runs short inside f must not drop_parked (it would also
  // wait for this lock for ever).
  template <class F>
  auto with_entries(F &&f) {
    std::lock_guard<std::mutex> lk(mu_);
    busy_ = true;   // (f does not throw)
    auto r = f(const_cast<const Map &>(map_));
    busy_ = false;
    return r;
  }
  bool busy() const { return busy_; }
  void free_unowned(H *h) { free_(h); }   // a handle that never went in (insert_if_absent gave it back)

 private:
  template <class P>
  void erase_if(P &&pred) {   // a held handle that leaves is its holder's to free
    for (auto it = map_.begin(); it != map_.end();) {
      H *h = it->second;
      if (!pred(it->first, h)) { ++it; continue; }
      it = map_.erase(it);
      h->cached = false;
      if (h->refcount == 0) free_(h);
    }
  }
  std::mutex mu_;
  Map map_;
  uint64_t clock_ = 0;   // release order of the parked handles
  std::atomic<bool> busy_{false};
  const std::function<void(H *)> free_;
  const int max_parked_;
};

// The Store worker: ONE thread builds every Store, one at a time, in the order they were asked for.  `Work` is what a build needs
// beside the key (default-constructed in the job, filled by the caller of get when the job is new, destroyed with the job).
// build(job, stream) -> rc: 0 with job.handle (refcount 0) set, or non-zero with the error text in job.err; `stream` is whatever
// start()'s setup handed over.  An object of this class lives on the heap and is never destroyed (see mpg_api.hip).
template <class H, class Work>
class StoreQueue {
 public:
  struct Job {
    StoreKey key;
    Work work;
    H *handle = nullptr;
    bool done = false;
    int rc = 0;
    std::string err;
  };
  typedef std::function<int(Job &, void *stream)> Build;
  StoreQueue(StoreCache<H> &cache, Build build) : cache_(cache), build_(std::move(build)) {}

  // Starts the worker unless it runs.  setup(&stream) -> rc runs first, on the caller's thread; bind(err) -> rc runs first on the
  // worker's.  A worker whose bind failed keeps serving the queue -- with that rc and text: a thread that simply left would make every
  // later Store wait for ever on a job nobody runs.
  int start(const std::function<int(void **stream)> &setup, std::function<int(std::string &err)> bind) {
    std::lock_guard<std::mutex> lk(start_mu_);
    if (thread_) return 0;
    int rc = setup(&stream_);
    if (rc) return rc;
    stop_ = false;
    thread_ = new std::thread(&StoreQueue::run, this, std::move(bind));
    return 0;
  }
  // The handle of `key`.  out != nullptr: -> 0 and *out with a reference for the caller, from the cache, or after waiting for the
  // key's job (joined if one is pending, else queued here; fill(job) completes a new one); a job's rc and text (*err) are every
  // waiter's.  A finished handle that has left the cache again before it was collected is built once more, once: then -> 0 with
  // *out == nullptr.  out == nullptr: make sure the key is cached, pending or queued, and return.
  int get(const StoreKey &key, H **out, const std::function<void(Job &)> &fill, std::string *err) {
    if (out) *out = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
      std::unique_lock<std::mutex> lk(mu_);
      if (out ? (*out = cache_.find_ref(key)) != nullptr : cache_.contains(key)) return 0;
      std::shared_ptr<Job> job;
      auto pit = pending_.find(key);
      if (pit != pending_.end()) {
        job = pit->second;
      } else {
        job = std::make_shared<Job>();
        job->key = key;
        fill(*job);
        pending_[key] = job;
        queue_.push_back(job);
      }
      cv_.notify_all();
      if (!out) return 0;
      cv_.wait(lk, [&] { return job->done; });
      if (job->rc) {
        if (err) *err = job->err;
        return job->rc;
      }
    }
    return 0;
  }
  void drain() {   // every queued / running Store has finished when this returns
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return pending_.empty(); });
  }
  void *stop() {   // drains first; -> the stream of setup, for the caller to dispose of (nullptr: no worker ran)
    std::lock_guard<std::mutex> slk(start_mu_);
    if (!thread_) return nullptr;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return pending_.empty(); });
      stop_ = true;
    }
    cv_.notify_all();
    thread_->join();
    delete thread_;
    thread_ = nullptr;
    void *s = stream_;
    stream_ = nullptr;
    return s;
  }

 private:
  void run(std::function<int(std::string &)> bind) {
    std::string bind_err;
    const int bind_rc = bind ? bind(bind_err) : 0;
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || !queue_.empty(); });
        if (queue_.empty()) return;   // stop asked and nothing left
        job = queue_.front();
        queue_.pop_front();
      }
      int rc = bind_rc;
      if (bind_rc) job->err = bind_err;
      else rc = build_(*job, stream_);
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (!rc && job->handle) {
          H *spare = cache_.insert_if_absent(job->key, job->handle);
          if (spare) cache_.free_unowned(spare);
        }
        job->handle = nullptr;
        job->rc = rc;
        job->done = true;
        pending_.erase(job->key);
      }
      cv_.notify_all();
    }
  }
  StoreCache<H> &cache_;
  const Build build_;
  std::mutex mu_, start_mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Job>> queue_;
  std::map<StoreKey, std::shared_ptr<Job>> pending_;   // queued or running
  std::thread *thread_ = nullptr;
  void *stream_ = nullptr;
  bool stop_ = false;
};
