// C-ABI entry points of libmpassit_amd.so (declared in include/mpassit_amd.h).
// Thin glue: argument checks, object lifetime, handle cache, host<->device staging.  All arithmetic is
// in the k_*.hip kernels; there is deliberately no CPU code path.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <cmath>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "compose_checks.h"
#include "mpg_internal.h"
#include "patch.h"
#include "creep.h"
#include "wind_reconstruct_checks.h"
#include "wind_vector_checks.h"

static thread_local char g_err[1024] = "";
static bool g_init = false;
static int g_device = -1;
static hipStream_t g_stream = nullptr;
// Released handles stay in the cache ("parked", refcount 0; StoreCache, store_cache.h) until their mesh or grid is destroyed, the
// library is finalized or more than MPG_MAX_PARKED of them wait: the reference stores the SAME element -> CENTER bilinear weights in
// interp_diag_data and again in interp_hist_data with a release in between (interp.F90:123,148 and :207), and a second
// mpg_regrid_store of a released key was a second run of the rasteriser (r02j: 2 x k_tri_raster in one job).
#define MPG_MAX_PARKED 8
static void handle_free(mpg_handle_s *h);
static StoreCache<mpg_handle_s> &cache() {   // on the heap, never destroyed: the Store worker below holds a reference to it
  static StoreCache<mpg_handle_s> *c = new StoreCache<mpg_handle_s>(handle_free, MPG_MAX_PARKED);
  return *c;
}
static void store_worker_drain();   // below: every queued / running Store has finished when this returns
static void store_worker_stop();
static int store_worker_start(int device);

void mpg_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
bool mpg_is_initialized() { return g_init; }
hipStream_t mpg_setup_stream() { return g_stream; }
int mpg_device_index() { return g_device; }

void mpg_cache_detach(mpg_handle_s *h) { cache().detach(h); }

// ---- cache of temporary device blocks (TmpBuf::alloc(count, stream), mpg_internal.h) ------------------------------------
namespace {
struct PoolBlock { void *p; size_t bytes; hipStream_t stream; };
std::vector<PoolBlock> g_pool;
std::mutex g_pool_mu;
size_t g_pool_bytes = 0;
const size_t POOL_CAP_BYTES = (size_t)4 << 30;   // beyond this a returned block goes straight back to the driver
}  // namespace

void *mpg_pool_get(size_t bytes, hipStream_t s) {
  bytes = (bytes + 255) & ~(size_t)255;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int best = -1;
    for (int i = 0; i < (int)g_pool.size(); ++i) {
      const PoolBlock &b = g_pool[i];
      if (b.stream != s || b.bytes < bytes || b.bytes > 2 * bytes + (1 << 20)) continue;   // same stream only; bounded waste
      if (best < 0 || b.bytes < g_pool[best].bytes) best = i;
    }
    if (best >= 0) {
      void *p = g_pool[best].p;
      g_pool_bytes -= g_pool[best].bytes;
      g_pool.erase(g_pool.begin() + best);
      return p;
    }
  }
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {   // the cache may be what fills the device: drop it and try once more
    mpg_pool_release();
    e = hipMalloc(&p, bytes);
  }
  if (e != hipSuccess) {
    mpg_set_error("HIP error %s allocating %zu bytes of scratch", hipGetErrorString(e), bytes);
    return nullptr;
  }
  return p;
}

// The size a block is cached under is the size it was ASKED with, rounded as mpg_pool_get rounds: a block found in the
// cache for a smaller request keeps its real size only if the caller returns it under that request's size -- so the cache
// tracks the real size itself.
static std::unordered_map<void *, size_t> g_pool_real;

void mpg_pool_put(void *p, size_t bytes, hipStream_t s) {
  if (!p) return;
  bytes = (bytes + 255) & ~(size_t)255;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  auto it = g_pool_real.find(p);
  if (it != g_pool_real.end()) bytes = it->second;
  else g_pool_real[p] = bytes;
  if (g_pool_bytes + bytes > POOL_CAP_BYTES) {
    g_pool_real.erase(p);
    (void)hipFree(p);
    return;
  }
  g_pool.push_back(PoolBlock{p, bytes, s});
  g_pool_bytes += bytes;
}

void mpg_pool_release() {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (const PoolBlock &b : g_pool) (void)hipFree(b.p);
  g_pool.clear();
  g_pool_real.clear();
  g_pool_bytes = 0;
}


// ---- first-call costs paid at mpg_init ---------------------------------------------------------------------------------
// The HIP runtime loads a translation unit's code object at the first launch of one of its kernels: measured on MI355X
// (tools/first_call_probe.py, profiles/r04_first_call.txt) the first nearest Store of a process took 8.0 ms against 3.1 ms
// for the second, the first conservative Store 14.5 against 4.5, the first mpg_mesh_create 12.5 against 4.5 -- MPASSIT is
// a single-shot tool (mpassit.F90:105-137), so the first values are what a run pays.  mpg_init therefore starts a helper
// thread that asks the runtime for one kernel of every translation unit (hipFuncGetAttributes loads the module) and
// creates the pinned staging of the host-array upload path, while the caller goes on (reading its namelist, opening its
// files); a call that needs a module before the helper got to it simply loads it itself (the runtime serialises that).
#define MPG_ANCHORS(X) X(k_setup) X(k_target_grid) X(k_store_bilinear) X(k_store_nearest) X(k_store_conserve) X(k_store_gridbil) \
  X(k_apply) X(k_apply_lfu) X(k_apply_typed) X(k_wind) X(k_pole) X(k_post) X(k_halo) X(mpg_comm) X(k_mesh_window) X(k_prims) X(k_sort) \
  X(k_transpose) X(k_apply_masked) X(k_store_to_mesh) X(k_apply_to_mesh) X(k_apply_csr_to_mesh) \
  X(k_store_mesh) X(k_apply_rows) X(k_store_conserve_mesh) X(k_apply_csr_rows) X(k_store_periodic_to_mesh) X(k_wind_pair) \
  X(k_wind_csr) X(k_wind_vector) X(k_wind_reconstruct) X(k_compose) X(k_wind_transpose) X(k_transpose_masked) X(k_extrapolate) \
  X(k_handle_mask) X(k_patch) X(k_conserve2nd) X(k_creep) X(k_store_conserve_grid) X(k_store_dtos)
#define X(n) const void *mpg_anchor_##n();
MPG_ANCHORS(X)
#undef X
static std::thread *g_warm = nullptr;   // on the heap: a process that exits without mpg_finalize must not meet ~thread of a joinable thread
// MPG_INIT_TRACE=1: where mpg_init's time and the helper thread's go, one line per step on stderr (tools/first_call_probe.py;
// profiles/r05_init_breakdown.md)
static bool g_init_trace = false;
static double now_ms() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}
static void warm_modules(int device) {
  if (hipSetDevice(device) != hipSuccess) return;
  (void)store_worker_start(device);   // the Store worker's thread and stream exist before the first RegridStore asks for them
  hipFuncAttributes a;
  double t0 = now_ms();
#define X(n)                                                                                                          \
  (void)hipFuncGetAttributes(&a, mpg_anchor_##n());                                                                   \
  if (g_init_trace) {                                                                                                 \
    const double t1 = now_ms();                                                                                       \
    fprintf(stderr, "mpg_init trace: helper thread: code object of %-18s %8.2f ms\n", #n, t1 - t0);                   \
    t0 = t1;                                                                                                          \
  }
  MPG_ANCHORS(X)
#undef X
  // the runtime builds its staging for copies from pageable host memory at the first such copy (9.5 ms in front of the first
  // mpg_mesh_create, rocprofv3 --hip-trace): one throw-away 32 MB upload does that here
  const size_t n = (size_t)32 << 20;
  void *h = malloc(n), *d = nullptr;
  hipStream_t s = nullptr;
  if (h && hipMalloc(&d, n) == hipSuccess && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess) {
    memset(h, 0, n);
    (void)hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s);
    (void)hipStreamSynchronize(s);
  }
  if (s) (void)hipStreamDestroy(s);
  if (d) (void)hipFree(d);
  free(h);
  if (g_init_trace) fprintf(stderr, "mpg_init trace: helper thread: first pageable 32 MB upload + its buffers %8.2f ms\n", now_ms() - t0);
}
static void warm_join() {   // mpg_finalize, and atexit (registered after the HIP runtime's own handlers: runs before them)
  if (g_warm) {
    if (g_warm->joinable()) g_warm->join();
    delete g_warm;
    g_warm = nullptr;
  }
}

// Everything the library holds only as a cache goes back to the driver: parked handles, scratch blocks.  Called when an
// allocation fails, before it is tried once more (DevBuf::alloc, mpg_dev_alloc).
void mpg_release_caches() {
  if (!cache().busy()) cache().drop_parked();
  mpg_pool_release();
}

extern "C" {

const char *mpg_last_error(void) { return g_err; }

int mpg_init(int device) {
  int n = 0;
  {
    const char *tr = getenv("MPG_INIT_TRACE");
    g_init_trace = tr && *tr == '1';
  }
  const double t_0 = now_ms();
  hipError_t e = hipGetDeviceCount(&n);
  const double t_1 = now_ms();
  if (e != hipSuccess || n <= 0) {
    mpg_set_error("mpg_init: no HIP device available (%s); this library has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return MPG_ERR_NOT_INITIALIZED;
  }
  MPG_ARG(device >= 0 && device < n, "mpg_init: device index out of range");
  if (g_init && device != g_device) {
    // the set-up stream, the file-io lanes and their pinned buffers belong to the first device; objects created there would
    // be paired with a stream of another device.  One device per process (one process per GPU); finalize first to switch.
    mpg_set_error("mpg_init: already initialised on device %d; call mpg_finalize before initialising device %d", g_device, device);
    return MPG_ERR_INVALID_ARG;
  }
  MPG_HIP(hipSetDevice(device));
  const double t_2 = now_ms();
  if (!g_init) {
    MPG_HIP(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    if (g_init_trace)
      fprintf(stderr, "mpg_init trace: hipGetDeviceCount (runtime start) %.2f ms, hipSetDevice %.2f ms, stream %.2f ms\n", t_1 - t_0, t_2 - t_1,
              now_ms() - t_2);
    const char *e = getenv("MPG_NO_WARMUP");   // A/B runs of the first-call probe
    if (!(e && *e == '1')) {
      g_warm = new std::thread(warm_modules, device);
      static bool registered = false;
      if (!registered) {
        atexit(warm_join);
        registered = true;
      }
    }
  }
  g_device = device;
  g_init = true;
  return MPG_SUCCESS;
}

// The helper thread of mpg_init allocates, frees and copies while it runs; a caller that starts a GLOBAL-mode stream capture right
// after mpg_init (hipStreamBeginCapture forbids such calls from other threads while it lasts) waits for it here first.
int mpg_warmup_wait(void) {
  warm_join();
  store_worker_drain();   // ... and for the Store worker (mpg_regrid_store_begin): it allocates too
  return MPG_SUCCESS;
}

int mpg_finalize(void) {
  if (!g_init) return MPG_SUCCESS;
  warm_join();
  store_worker_stop();
  cache().drop_parked();
  mpg_fileio_release();
  mpg_hostpipe_release();
  (void)hipStreamSynchronize(g_stream);
  mpg_pool_release();
  (void)hipStreamDestroy(g_stream);
  g_stream = nullptr;
  g_init = false;
  return MPG_SUCCESS;
}

// GPUs this process can see; may be called before mpg_init (a launcher's ranks pick their device with it)
int mpg_device_count(int *n) {
  MPG_ARG(n, "mpg_device_count: NULL argument");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return MPG_SUCCESS;
}

int mpg_device_info(char *arch_buf, int buf_len, int *n_cu, int64_t *hbm_bytes) {
  MPG_CHECK_INIT();
  hipDeviceProp_t p;
  MPG_HIP(hipGetDeviceProperties(&p, g_device));
  if (arch_buf && buf_len > 0) {
    strncpy(arch_buf, p.gcnArchName, (size_t)buf_len - 1);
    arch_buf[buf_len - 1] = 0;
  }
  if (n_cu) *n_cu = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return MPG_SUCCESS;
}

// ---- mesh -----------------------------------------------------------------------------------------
static std::vector<mpg_mesh_s *> g_meshes;   // live meshes: a grid that goes away tells the meshes cut to it (geo_grid)

static int mesh_common_checks(int64_t nCells, int64_t nVertices, int maxEdges, const double *latCell, const double *lonCell, const double *latVertex,
                              const double *lonVertex, const int32_t *verticesOnCell, mpg_mesh *out, const char *who) {
  if (!out) { mpg_set_error("%s: out is NULL", who); return MPG_ERR_INVALID_ARG; }
  if (!(nCells > 0 && nVertices > 0 && maxEdges >= 3)) { mpg_set_error("%s: nCells, nVertices must be > 0 and maxEdges >= 3", who); return MPG_ERR_INVALID_ARG; }
  if (!(nCells < 0x7fffffff && nVertices < 0x7fffffff)) { mpg_set_error("%s: sizes must fit int32 ids", who); return MPG_ERR_INVALID_ARG; }
  if (!(latCell && lonCell && latVertex && lonVertex && verticesOnCell)) { mpg_set_error("%s: NULL array", who); return MPG_ERR_INVALID_ARG; }
  return MPG_SUCCESS;
}

// ESMF_MeshCreate for ONE rank of a row-sharded job (include/mpassit_amd.h; k_mesh_window.hip has the method and the argument
// why the weights equal those of the whole mesh)
int mpg_mesh_create_window(int64_t nCells, int64_t nVertices, int maxEdges, const double *latCell, const double *lonCell, const double *latVertex,
                           const double *lonVertex, const int32_t *verticesOnCell, mpg_grid grid, mpg_mesh *out) {
  MPG_CHECK_INIT();
  int rc = mesh_common_checks(nCells, nVertices, maxEdges, latCell, lonCell, latVertex, lonVertex, verticesOnCell, out, "mpg_mesh_create_window");
  if (rc) return rc;
  MPG_ARG(grid, "mpg_mesh_create_window: NULL grid");
  mpg_mesh_s *m = new mpg_mesh_s();
  m->nCells = nCells;
  m->nVertices = nVertices;
  m->maxEdges = maxEdges;
  m->geo_grid = grid;
  g_meshes.push_back(m);
  store_worker_drain();   // mpg_k_mesh_window builds and reads grid->pyr[] / cellpyr: a begun Store on this grid builds them on the worker
  if ((rc = mpg_k_mesh_coords(nCells, lonCell, latCell, m->cell, g_stream)) ||
      (rc = mpg_k_mesh_window(m, grid, latVertex, lonVertex, verticesOnCell, g_stream))) {
    mpg_mesh_destroy(m);
    return rc;
  }
  *out = m;
  return MPG_SUCCESS;
}

int mpg_mesh_window_info(mpg_mesh m, int64_t *cell_first, int64_t *cell_count, int64_t *vertex_first, int64_t *vertex_count, double *margin) {
  MPG_ARG(m, "mpg_mesh_window_info: NULL mesh");
  if (cell_first) *cell_first = m->cw0;
  if (cell_count) *cell_count = m->cwn;
  if (vertex_first) *vertex_first = m->vw0;
  if (vertex_count) *vertex_count = m->vwn;
  if (margin) *margin = m->geo_margin;
  return MPG_SUCCESS;
}

int mpg_mesh_create(int64_t nCells, int64_t nVertices, int maxEdges, const double *latCell, const double *lonCell,
                    const double *latVertex, const double *lonVertex, const int32_t *verticesOnCell, mpg_mesh *out) {
  MPG_CHECK_INIT();
  {
    int rc0 = mesh_common_checks(nCells, nVertices, maxEdges, latCell, lonCell, latVertex, lonVertex, verticesOnCell, out, "mpg_mesh_create");
    if (rc0) return rc0;
  }
  mpg_mesh_s *m = new mpg_mesh_s();
  m->nCells = nCells;
  m->nVertices = nVertices;
  m->maxEdges = maxEdges;
  m->cwn = nCells;      // geometry window = the whole mesh
  m->vwn = nVertices;
  m->geo_margin = 4.0;
  g_meshes.push_back(m);
  int rc;
  hipStream_t s = g_stream;
  if ((rc = mpg_k_mesh_coords(nCells, lonCell, latCell, m->cell, s)) || (rc = mpg_k_mesh_coords(nVertices, lonVertex, latVertex, m->vert, s)) ||
      (rc = m->voc.alloc((size_t)nCells * maxEdges))) {
    mpg_mesh_destroy(m);
    return rc;
  }
  hipError_t he = hipMemcpyAsync(m->voc.p, verticesOnCell, sizeof(int32_t) * (size_t)nCells * maxEdges, hipMemcpyHostToDevice, s);
  if (he != hipSuccess) {
    mpg_set_error("mpg_mesh_create: uploading verticesOnCell failed: %s", hipGetErrorString(he));
    mpg_mesh_destroy(m);
    return MPG_ERR_HIP;
  }
  if ((rc = mpg_k_voc_check(m->voc.p, nCells * maxEdges, nVertices, "mpg_mesh_create", s)) || (rc = mpg_k_dual_triangles(m, s))) {
    mpg_mesh_destroy(m);
    return rc;
  }
  *out = m;
  return MPG_SUCCESS;
}

// handles outlive neither their mesh nor their grid in the cache: a recycled address must never hit
static void cache_purge(void *obj) {
  store_worker_drain();   // a Store in flight reads the mesh and the grid it was started on
  cache().purge(obj);
}

int mpg_mesh_destroy(mpg_mesh m) {
  if (!m) return MPG_SUCCESS;
  cache_purge(m);
  for (size_t i = 0; i < g_meshes.size(); ++i)
    if (g_meshes[i] == m) {
      g_meshes.erase(g_meshes.begin() + (long)i);
      break;
    }
  m->cell.free();
  m->vert.free();
  m->edge.free();
  m->angle_edge.free();
  m->voc.free();
  m->tri.free();
  m->fan.free();
  m->bvh.free();
  m->tbvh.free();
  m->cbvh.free();
  delete m;
  return MPG_SUCCESS;
}

// The mesh's edge points (MPG_MESHLOC_EDGE): a third PointSet through the cell centres' conversion, angleEdge kept as given.  Once per
// mesh, so that handles onto the edges -- cached ones included -- never outlive the points they were stored for.
int mpg_mesh_set_edges(mpg_mesh m, int64_t nEdges, const double *latEdge, const double *lonEdge, const double *angleEdge) {
  MPG_CHECK_INIT();
  MPG_ARG(m, "mpg_mesh_set_edges: NULL mesh");
  if (m->geo_grid) {
    mpg_set_error("mpg_mesh_set_edges: the mesh was cut to a grid (mpg_mesh_create_window): its resident points are a window; "
                  "create the whole mesh (mpg_mesh_create) for results on its edges");
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG(m->edge.n == 0, "mpg_mesh_set_edges: edges are already set on this mesh (handles onto them stay valid; create another mesh for other edges)");
  MPG_ARG(nEdges >= 1, "mpg_mesh_set_edges: nEdges must be >= 1");
  if (nEdges >= 0x7fffffff) {
    mpg_set_error("mpg_mesh_set_edges: %lld edges exceed int32 ids", (long long)nEdges);
    return MPG_ERR_OVERFLOW;
  }
  MPG_ARG(latEdge && lonEdge, "mpg_mesh_set_edges: NULL coordinates (latEdge, lonEdge)");
  if (angleEdge)
    for (int64_t i = 0; i < nEdges; ++i)
      if (!std::isfinite(angleEdge[i])) {
        mpg_set_error("mpg_mesh_set_edges: angleEdge of edge %lld is %.17g -- not an angle in RADIANS (finite)", (long long)i, angleEdge[i]);
        return MPG_ERR_INVALID_ARG;
      }
  hipStream_t s = g_stream;
  PointSet pts;
  DevBuf<double> ang;
  int rc = mpg_k_mesh_coords(nEdges, lonEdge, latEdge, pts, s);   // synchronises: the host arrays are free on return
  if (!rc && angleEdge && !(rc = ang.alloc((size_t)nEdges))) {
    hipError_t he = hipMemcpyAsync(ang.p, angleEdge, sizeof(double) * (size_t)nEdges, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) {
      mpg_set_error("mpg_mesh_set_edges: uploading angleEdge failed: %s", hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  if (rc) {   // the mesh stays without edges
    pts.free();
    ang.free();
    return rc;
  }
  // (no drain: a Store onto edges is refused until they are set and they are set once, so no begun Store reads m->edge)
  m->edge = pts;
  m->angle_edge = ang;
  return MPG_SUCCESS;
}

int mpg_mesh_edge_count(mpg_mesh m, int64_t *nEdges) {
  MPG_ARG(m && nEdges, "mpg_mesh_edge_count: NULL argument");
  *nEdges = m->edge.n;
  return MPG_SUCCESS;
}

int mpg_mesh_get_triangles(mpg_mesh m, int32_t *tri_host) {
  MPG_CHECK_INIT();
  MPG_ARG(m && tri_host, "mpg_mesh_get_triangles: NULL argument");
  const int64_t nV = m->vwn;   // vertices outside the geometry window of a mesh cut to a grid have no triangle here
  for (int64_t i = 0; i < 3 * m->nVertices; ++i) tri_host[i] = -1;
  if (nV == 0) return MPG_SUCCESS;
  std::vector<int32_t> tmp(3 * (size_t)nV);
  MPG_HIP(hipMemcpy(tmp.data(), m->tri.p, sizeof(int32_t) * 3 * nV, hipMemcpyDeviceToHost));
  for (int64_t v = 0; v < nV; ++v)
    for (int k = 0; k < 3; ++k) tri_host[3 * (m->vw0 + v) + k] = tmp[(size_t)k * nV + v];
  return MPG_SUCCESS;
}

// the stored unit vectors of a point set, [3][n] on the host: the bits every search of this library uses
static int get_xyz(const char *who, const PointSet &pts, int64_t n, double *xyz_host) {
  if (pts.n != n || n == 0) {
    if (n == 0) return MPG_SUCCESS;
    mpg_set_error("%s: the location has no coordinates", who);
    return MPG_ERR_INVALID_ARG;
  }
  MPG_HIP(hipMemcpy(xyz_host, pts.x.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  MPG_HIP(hipMemcpy(xyz_host + n, pts.y.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  MPG_HIP(hipMemcpy(xyz_host + 2 * n, pts.z.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

int mpg_mesh_get_xyz(mpg_mesh m, int meshloc, double *xyz_host) {
  MPG_CHECK_INIT();
  MPG_ARG(m && xyz_host, "mpg_mesh_get_xyz: NULL argument");
  MPG_ARG(meshloc == MPG_MESHLOC_ELEMENT || meshloc == MPG_MESHLOC_NODE || meshloc == MPG_MESHLOC_EDGE, "mpg_mesh_get_xyz: bad mesh location");
  MPG_ARG(meshloc != MPG_MESHLOC_NODE || m->vwn == m->nVertices,
          "mpg_mesh_get_xyz: the vertices of a mesh cut to a grid (mpg_mesh_create_window) are not all resident");
  const PointSet &pts = meshloc == MPG_MESHLOC_EDGE ? m->edge : meshloc == MPG_MESHLOC_ELEMENT ? m->cell : m->vert;
  const int64_t n = meshloc == MPG_MESHLOC_EDGE ? m->edge.n : meshloc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
  return get_xyz("mpg_mesh_get_xyz", pts, n, xyz_host);
}

// ---- grid -----------------------------------------------------------------------------------------
int mpg_grid_get_xyz(mpg_grid g, int staggerloc, double *xyz_host) {
  MPG_CHECK_INIT();
  MPG_ARG(g && xyz_host, "mpg_grid_get_xyz: NULL argument");
  MPG_ARG(staggerloc >= 0 && staggerloc < 4, "mpg_grid_get_xyz: bad stagger location");
  return get_xyz("mpg_grid_get_xyz", g->pts[staggerloc], (int64_t)g->snx[staggerloc] * g->sny[staggerloc], xyz_host);
}

int mpg_grid_create(int nx, int ny, int periodic_i, const double *lon_center, const double *lat_center, const double *lon_corner,
                    const double *lat_corner, const double *lon_edge1, const double *lat_edge1, const double *lon_edge2,
                    const double *lat_edge2, mpg_grid *out) {
  MPG_CHECK_INIT();
  MPG_ARG(out, "mpg_grid_create: out is NULL");
  MPG_ARG(nx > 0 && ny > 0, "mpg_grid_create: nx, ny must be > 0");
  MPG_ARG(lon_center && lat_center, "mpg_grid_create: CENTER coordinates are mandatory");
  MPG_ARG(periodic_i >= 0 && periodic_i < 8 && ((periodic_i & MPG_GRID_PERIODIC_I) || !periodic_i),
          "mpg_grid_create: periodic_i must be 0 or MPG_GRID_PERIODIC_I [| MPG_GRID_NO_SOUTH_POLE | MPG_GRID_NO_NORTH_POLE]");
  MPG_ARG((int64_t)(nx + 1) * (ny + 1) < 0x7fffffff, "mpg_grid_create: grid too large for int32 ids");
  mpg_grid_s *g = new mpg_grid_s();
  g->nx = nx;
  g->ny = ny;
  g->periodic = periodic_i;
  g->snx[MPG_STAGGERLOC_CENTER] = nx;     g->sny[MPG_STAGGERLOC_CENTER] = ny;
  g->snx[MPG_STAGGERLOC_EDGE1] = nx + 1;  g->sny[MPG_STAGGERLOC_EDGE1] = ny;
  g->snx[MPG_STAGGERLOC_EDGE2] = nx;      g->sny[MPG_STAGGERLOC_EDGE2] = ny + 1;
  g->snx[MPG_STAGGERLOC_CORNER] = nx + 1; g->sny[MPG_STAGGERLOC_CORNER] = ny + 1;
  const double *lon[4] = {lon_center, lon_edge1, lon_edge2, lon_corner};
  const double *lat[4] = {lat_center, lat_edge1, lat_edge2, lat_corner};
  for (int st = 0; st < 4; ++st) {
    if (!lon[st] || !lat[st]) continue;
    int rc = mpg_k_grid_coords((int64_t)g->snx[st] * g->sny[st], lon[st], lat[st], g->pts[st], g_stream);
    if (rc) {
      mpg_grid_destroy(g);
      return rc;
    }
  }
  *out = g;
  return MPG_SUCCESS;
}

int mpg_grid_destroy(mpg_grid g) {
  if (!g) return MPG_SUCCESS;
  cache_purge(g);
  for (mpg_mesh_s *m : g_meshes)   // a mesh cut to this grid serves no other: a recycled address must never pass for it
    if (m->geo_grid == g) m->geo_grid_gone = true;
  for (int st = 0; st < 4; ++st) {
    g->pts[st].free();
    g->pyr[st].free();
  }
  g->cellpyr.free();
  for (int st = 0; st < 4; ++st) g->quadpyr[st].free();
  g->wrappyr.free();
  for (int st = 0; st < 4; ++st) {
    g->lon[st].free();
    g->lat[st].free();
  }
  for (int st = 0; st < 3; ++st) g->mapfac[st].free();
  g->cosa.free();
  g->sina.free();
  delete g;
  return MPG_SUCCESS;
}

static void grid_shape(mpg_grid_s *g, int nx, int ny, int periodic_i) {
  g->nx = nx;
  g->ny = ny;
  g->periodic = periodic_i;
  g->snx[MPG_STAGGERLOC_CENTER] = nx;     g->sny[MPG_STAGGERLOC_CENTER] = ny;
  g->snx[MPG_STAGGERLOC_EDGE1] = nx + 1;  g->sny[MPG_STAGGERLOC_EDGE1] = ny;
  g->snx[MPG_STAGGERLOC_EDGE2] = nx;      g->sny[MPG_STAGGERLOC_EDGE2] = ny + 1;
  g->snx[MPG_STAGGERLOC_CORNER] = nx + 1; g->sny[MPG_STAGGERLOC_CORNER] = ny + 1;
}

int mpg_grid_create_proj(const mpg_proj *proj, int nx, int ny, int periodic_i, mpg_grid *out) {
  MPG_CHECK_INIT();
  MPG_ARG(proj && out, "mpg_grid_create_proj: NULL argument");
  MPG_ARG(nx > 0 && ny > 0, "mpg_grid_create_proj: nx, ny must be > 0");
  MPG_ARG((int64_t)(nx + 1) * (ny + 1) < 0x7fffffff, "mpg_grid_create_proj: grid too large for int32 ids");
  MPG_ARG(periodic_i >= 0 && periodic_i < 8 && ((periodic_i & MPG_GRID_PERIODIC_I) || !periodic_i),
          "mpg_grid_create_proj: periodic_i must be 0 or MPG_GRID_PERIODIC_I [| MPG_GRID_NO_SOUTH_POLE | MPG_GRID_NO_NORTH_POLE]");
  mpg_grid_s *g = new mpg_grid_s();
  grid_shape(g, nx, ny, periodic_i);
  int rc = mpg_k_target_grid(proj, g, g_stream);
  if (rc) {
    mpg_grid_destroy(g);
    return rc;
  }
  *out = g;
  return MPG_SUCCESS;
}

int mpg_grid_attach_proj(mpg_grid g, const mpg_proj *proj, int row0) {
  MPG_CHECK_INIT();
  MPG_ARG(g && proj, "mpg_grid_attach_proj: NULL argument");
  MPG_ARG(row0 >= 0, "mpg_grid_attach_proj: row0 must be >= 0");
  store_worker_drain();   // a begun Store on this grid reads g->proj / has_inverse to choose its candidate search
  return mpg_k_attach_proj(g, proj, row0, g_stream);
}

#define MPG_PROJ_GRID(g, what)                                                                  \
  do {                                                                                          \
    MPG_ARG(g, what ": NULL grid");                                                             \
    if (!(g)->from_proj) {                                                                      \
      mpg_set_error(what ": the grid was created from caller arrays (mpg_grid_create), which the caller still holds"); \
      return MPG_ERR_UNSUPPORTED;                                                               \
    }                                                                                           \
  } while (0)

int mpg_grid_get_coords(mpg_grid g, int staggerloc, double *lon_host, double *lat_host) {
  MPG_CHECK_INIT();
  MPG_PROJ_GRID(g, "mpg_grid_get_coords");
  MPG_ARG(staggerloc >= 0 && staggerloc < 4, "mpg_grid_get_coords: bad staggerloc");
  size_t bytes = sizeof(double) * (size_t)g->snx[staggerloc] * g->sny[staggerloc];
  if (lon_host) MPG_HIP(hipMemcpy(lon_host, g->lon[staggerloc].p, bytes, hipMemcpyDeviceToHost));
  if (lat_host) MPG_HIP(hipMemcpy(lat_host, g->lat[staggerloc].p, bytes, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

int mpg_grid_get_mapfac(mpg_grid g, int staggerloc, double *mapfac_host) {
  MPG_CHECK_INIT();
  MPG_PROJ_GRID(g, "mpg_grid_get_mapfac");
  MPG_ARG(staggerloc >= 0 && staggerloc < 3 && mapfac_host, "mpg_grid_get_mapfac: CENTER, EDGE1 or EDGE2 and a buffer");
  MPG_HIP(hipMemcpy(mapfac_host, g->mapfac[staggerloc].p, sizeof(double) * (size_t)g->snx[staggerloc] * g->sny[staggerloc],
                    hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

int mpg_grid_rotang_dev(mpg_grid g, const double **cosa_dev, const double **sina_dev) {
  MPG_CHECK_INIT();
  MPG_PROJ_GRID(g, "mpg_grid_rotang_dev");
  if (!g->cosa.p) {
    mpg_set_error("mpg_grid_rotang_dev: cos/sin(alpha) exist for PROJ_LC grids only (model_grid.F90:1113)");
    return MPG_ERR_UNSUPPORTED;
  }
  if (cosa_dev) *cosa_dev = g->cosa.p;
  if (sina_dev) *sina_dev = g->sina.p;
  return MPG_SUCCESS;
}

int mpg_grid_get_rotang(mpg_grid g, double *cosa_host, double *sina_host) {
  const double *c, *s;
  int rc = mpg_grid_rotang_dev(g, &c, &s);
  if (rc) return rc;
  size_t bytes = sizeof(double) * (size_t)g->nx * g->ny;
  if (cosa_host) MPG_HIP(hipMemcpy(cosa_host, c, bytes, hipMemcpyDeviceToHost));
  if (sina_host) MPG_HIP(hipMemcpy(sina_host, s, bytes, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

// cos / sin of the rotation angle at the points of a mesh, for mpg_wind_to_mesh_dev (k_target_grid.hip k_mesh_rotang)
int mpg_mesh_rotang_dev(mpg_grid g, mpg_mesh mesh, int meshloc, double *cosa_dev, double *sina_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(g && mesh, "mpg_mesh_rotang: NULL grid or mesh");
  MPG_ARG(meshloc == MPG_MESHLOC_ELEMENT || meshloc == MPG_MESHLOC_NODE, "mpg_mesh_rotang: unknown mesh location (MPG_MESHLOC_ELEMENT or MPG_MESHLOC_NODE)");
  if (!g->has_inverse) {
    mpg_set_error("mpg_mesh_rotang: the grid carries no projection (mpg_grid_create_proj or mpg_grid_attach_proj give it one); "
                  "without one the forward chain does not rotate there: pass NULL angles");
    return MPG_ERR_UNSUPPORTED;
  }
  if (g->proj.code != MPG_PROJ_LC) {
    mpg_set_error("mpg_mesh_rotang: cos/sin(alpha) exist for PROJ_LC grids only (model_grid.F90:1113); "
                  "the forward chain does not rotate there: pass NULL angles");
    return MPG_ERR_UNSUPPORTED;
  }
  if (mesh->geo_grid) {
    mpg_set_error("mpg_mesh_rotang: the mesh was cut to a grid (mpg_mesh_create_window): its resident points are a window; "
                  "create the whole mesh (mpg_mesh_create) for results on the mesh");
    return MPG_ERR_UNSUPPORTED;
  }
  const PointSet &pts = meshloc == MPG_MESHLOC_ELEMENT ? mesh->cell : mesh->vert;
  MPG_ARG(pts.n == 0 || (cosa_dev && sina_dev), "mpg_mesh_rotang: NULL output");
  return mpg_k_mesh_rotang(g, pts.n, pts.x.p, pts.y.p, cosa_dev, sina_dev, (hipStream_t)hip_stream);
}

// cos / sin of phi = angleEdge - alpha at the edges of a mesh, for mpg_wind_to_edges_dev (k_target_grid.hip k_mesh_edge_rotang); a NULL
// grid: alpha = 0.  (A windowed mesh has no edges: mpg_mesh_set_edges refuses it.)
int mpg_mesh_edge_rotang_dev(mpg_grid g, mpg_mesh mesh, double *cn_dev, double *sn_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(mesh, "mpg_mesh_edge_rotang: NULL mesh");
  MPG_ARG(mesh->edge.n > 0, "mpg_mesh_edge_rotang: the mesh has no edges: mpg_mesh_set_edges gives it some");
  MPG_ARG(mesh->angle_edge.p, "mpg_mesh_edge_rotang: the mesh's edges carry no angleEdge: mpg_mesh_set_edges takes it with the coordinates");
  if (g && !g->has_inverse) {
    mpg_set_error("mpg_mesh_edge_rotang: the grid carries no projection (mpg_grid_create_proj or mpg_grid_attach_proj give it one); "
                  "without one the forward chain does not rotate there: pass a NULL grid");
    return MPG_ERR_UNSUPPORTED;
  }
  if (g && g->proj.code != MPG_PROJ_LC) {
    mpg_set_error("mpg_mesh_edge_rotang: cos/sin(alpha) exist for PROJ_LC grids only (model_grid.F90:1113); "
                  "the forward chain does not rotate there: pass a NULL grid");
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG(cn_dev && sn_dev, "mpg_mesh_edge_rotang: NULL output");
  const PointSet &pts = mesh->edge;
  return mpg_k_mesh_edge_rotang(g, pts.n, pts.x.p, pts.y.p, mesh->angle_edge.p, cn_dev, sn_dev, (hipStream_t)hip_stream);
}

// ---- RegridStore ----------------------------------------------------------------------------------
static void handle_free(mpg_handle_s *h) {
  h->idx.free();
  h->w.free();
  h->rowptr.free();
  h->col.free();
  h->val.free();
  h->dst_frac.free();
  h->src_nearest.free();
  h->pole_dst.free();
  h->pole_src0.free();
  h->pole_w.free();
  h->free_tile_lists();
  delete h;
}

struct StoreCtx {   // what a Store's build reads: the key's objects, typed by what its kind says they are
  mpg_mesh_s *src_mesh = nullptr, *dst_mesh = nullptr;
  mpg_grid_s *src_grid = nullptr, *dst_grid = nullptr;
  int src_loc, dst_loc;   // MPG_MESHLOC_* of a mesh, MPG_STAGGERLOC_* of a grid
  int method, pole_method, norm_type;
  explicit StoreCtx(const StoreKey &k) : src_loc(k.src_loc), dst_loc(k.dst_loc), method(k.method), pole_method(k.pole_method), norm_type(k.norm_type) {
    if (k.source_is_mesh()) src_mesh = (mpg_mesh_s *)k.src;
    else src_grid = (mpg_grid_s *)k.src;
    if (k.kind == STORE_MESH_TO_GRID || k.kind == STORE_GRID_TO_GRID || k.kind == STORE_GRID_TO_OTHER_GRID || k.kind == STORE_CONSERVE_GRID_TO_GRID)
      dst_grid = (mpg_grid_s *)k.dst;
    else dst_mesh = (mpg_mesh_s *)k.dst;
  }
};
typedef int (*StoreBuildFn)(mpg_handle_s *, const StoreCtx &, hipStream_t);
static StoreBuildFn store_build_fn(StoreKind kind);   // below, after the nine builds

// ---- the Store worker -------------------------------------------------------------------------------------------------
// interp.F90:207-437 stores its weight sets one after the other, each in front of the Regrids that use it; they are
// independent of each other and of every Regrid that does not use them.  All RegridStores of this library run on ONE worker
// thread with a stream of its own: mpg_regrid_store[_grid]_begin queues a Store and returns; mpg_regrid_store[_grid] returns
// the finished handle of its key -- from the cache, from the queue (waiting for it), or by queueing it itself and waiting.
// While the worker builds the conservative and nearest-neighbour weights (3 of the 4.6 ms of configuration 4's Stores,
// compute-bound kernels) the caller's thread is already issuing the bilinear Regrids (HBM-bound) on ITS stream.  One
// Store at a time: the lazily built search structures of a mesh / grid (pyramids, BVH, fans) are only ever touched by this
// thread, or by an entry point that has drained it first (mpg_mesh_create_window; DESIGN.md lists the entries).  The weights do not
// depend on which thread builds them.  The key, the cache and the queue are store_cache.h.
struct StoreWork {
  hipEvent_t ready = nullptr;   // recorded on the set-up stream when the job was queued: the mesh / grid uploads and kernels issued there come first
  ~StoreWork() {
    if (ready) (void)hipEventDestroy(ready);
  }
};
typedef StoreQueue<mpg_handle_s, StoreWork> StoreWorker;
static int store_build_now(StoreWorker::Job &job, void *stream);
// The worker's state lives on the heap and is never destroyed: a process that ends without mpg_finalize (a Fortran `stop`, an error exit)
// must not run the destructor of a condition variable the worker is waiting on (that blocks for ever).
static StoreWorker &SW() {
  static StoreWorker *w = new StoreWorker(cache(), store_build_now);
  return *w;
}

static int store_build(StoreWorker::Job &job, hipStream_t s) {
  mpg_handle_s *h = new mpg_handle_s();
  h->refcount = 0;   // nobody holds it yet: parked in the cache until a mpg_regrid_store collects it
  h->method = job.key.method;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    mpg_set_error("hipEventCreate failed in a RegridStore");
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, s);
  int rc = store_build_fn(job.key.kind)(h, StoreCtx(job.key), s);
  if (!rc) {
    hipError_t e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (e != hipSuccess) {
      mpg_set_error("RegridStore: %s", hipGetErrorString(e));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    handle_free(h);
    return rc;
  }
  job.handle = h;   // the worker parks it in the cache and leaves `pending` in one step (StoreQueue::run)
  return MPG_SUCCESS;
}
static int store_build_now(StoreWorker::Job &job, void *stream) {   // on the worker's thread; a failed job carries its error text
  g_err[0] = 0;
  if (job.work.ready) (void)hipStreamWaitEvent((hipStream_t)stream, job.work.ready, 0);
  const int rc = store_build(job, (hipStream_t)stream);
  if (rc) job.err = g_err;
  return rc;
}

static int store_worker_start(int device) {   // mpg_init's helper thread starts it; a Store that comes first starts it itself
  return SW().start(
      [](void **stream) -> int {
        MPG_HIP(hipStreamCreateWithFlags((hipStream_t *)stream, hipStreamNonBlocking));
        return MPG_SUCCESS;
      },
      [device](std::string &err) -> int {
        const hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) return MPG_SUCCESS;
        mpg_set_error("RegridStore: the Store worker could not bind device %d: %s", device, hipGetErrorString(e));
        err = g_err;
        return MPG_ERR_HIP;
      });
}
static void store_worker_drain() { SW().drain(); }
static void store_worker_stop() {   // mpg_finalize
  if (void *stream = SW().stop()) (void)hipStreamDestroy((hipStream_t)stream);
}

// out == nullptr: start the Store and return (mpg_regrid_store[_grid]_begin); else return the handle, waiting for its Store.  In use
// elsewhere, or parked by an earlier release / a finished _begin: the same weights, no device work.
static int store_common(const StoreKey &key, mpg_handle *out) {
  int rc = store_worker_start(g_device);
  if (rc) return rc;
  std::string err;
  rc = SW().get(key, out, [](StoreWorker::Job &job) {
    if (hipEventCreateWithFlags(&job.work.ready, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(job.work.ready, g_stream);
  }, &err);
  if (rc) {
    mpg_set_error("%s", err.c_str());
    return rc;
  }
  if (out && !*out) {   // a flood of releases has pushed the finished handle out again, twice
    mpg_set_error("RegridStore: the finished handle left the cache before it was collected");
    return MPG_ERR_HIP;
  }
  return MPG_SUCCESS;
}

// the source mesh's points are windowed (mpg_mesh_set_source_window): a new handle indexes relative to the window from the start
static int rebase_to_window(mpg_handle_s *h, const mpg_mesh_s *m, int loc, hipStream_t s) {
  return m->win_count[loc] >= 0 ? mpg_k_rebase(h, m->win_first[loc], m->win_count[loc], s, true) : (int)MPG_SUCCESS;
}
static int store_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  int rc;
  if (x.method == MPG_REGRIDMETHOD_BILINEAR) rc = mpg_k_store_bilinear_mesh(x.src_mesh, x.dst_grid, x.dst_loc, x.src_loc, h, s);
  else if (x.method == MPG_REGRIDMETHOD_NEAREST_STOD) rc = mpg_k_store_nearest(x.src_mesh, x.dst_grid, x.dst_loc, h, s);
  else rc = mpg_k_store_conserve(x.src_mesh, x.dst_grid, h, s);
  return rc ? rc : rebase_to_window(h, x.src_mesh, x.src_loc, s);
}
static int store_grid_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  return mpg_k_store_grid_bilinear(x.src_grid, x.dst_loc, h, s);
}

static int store_mesh_entry(mpg_mesh src, int src_meshloc, mpg_grid dst, int dst_staggerloc, int regridmethod, mpg_handle *out, const char *who) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst, "mpg_regrid_store: NULL argument");
  MPG_ARG(dst_staggerloc >= 0 && dst_staggerloc <= 2, "mpg_regrid_store: destination stagger must be CENTER, EDGE1 or EDGE2");
  MPG_ARG(src_meshloc == MPG_MESHLOC_ELEMENT || src_meshloc == MPG_MESHLOC_NODE, "mpg_regrid_store: unknown mesh location");
  if (src_meshloc == MPG_MESHLOC_NODE && regridmethod != MPG_REGRIDMETHOD_BILINEAR) {
    mpg_set_error("%s: node-located sources are only regridded bilinearly by the reference (interp.F90:350-366)", who);
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG(regridmethod >= 0 && regridmethod <= 2, "mpg_regrid_store: unknown regrid method");
  if (src->geo_grid && (src->geo_grid != dst || src->geo_grid_gone)) {
    mpg_set_error("%s: the mesh was cut to another grid (mpg_mesh_create_window%s); it holds only the cells that grid can see", who,
                  src->geo_grid_gone ? ", which has been destroyed" : "");
    return MPG_ERR_INVALID_ARG;
  }
  if (regridmethod == MPG_REGRIDMETHOD_CONSERVE && dst_staggerloc != MPG_STAGGERLOC_CENTER) {
    mpg_set_error("%s: conservative regridding is defined on the CENTER stagger only", who);
    return MPG_ERR_UNSUPPORTED;
  }
  // the line type in force is part of what a bilinear handle IS, and so is the apex rule of the polygon fans for node-located sources
  return store_common(StoreKey::mesh_to_grid(src, src_meshloc, dst, dst_staggerloc, regridmethod, mpg_bilinear_linetype(), mpg_node_fan_origin()), out);
}

int mpg_regrid_store(mpg_mesh src, int src_meshloc, mpg_grid dst, int dst_staggerloc, int regridmethod, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(out, "mpg_regrid_store: NULL argument");
  return store_mesh_entry(src, src_meshloc, dst, dst_staggerloc, regridmethod, out, "mpg_regrid_store");
}
int mpg_regrid_store_begin(mpg_mesh src, int src_meshloc, mpg_grid dst, int dst_staggerloc, int regridmethod) {
  return store_mesh_entry(src, src_meshloc, dst, dst_staggerloc, regridmethod, nullptr, "mpg_regrid_store_begin");
}

// ---- source window of a mesh (a host that holds only the cells its target rows reference) ---------------------------------
int mpg_handle_source_range(mpg_handle h, int64_t *first, int64_t *end) {
  MPG_CHECK_INIT();
  MPG_ARG(h && first && end, "mpg_handle_source_range: NULL argument");
  MPG_ARG(!h->localized, "mpg_handle_source_range: the handle was re-indexed (mpg_handle_localize / mpg_handle_rebase)");
  int rc = mpg_k_source_range(h, first, end, g_stream);
  if (rc) return rc;
  if (*end > *first) {   // a handle of a windowed mesh: back to global ids
    const int64_t w0 = mpg_handle_window_first(h);
    *first += w0;
    *end += w0;
  }
  return MPG_SUCCESS;
}

int mpg_mesh_set_source_window(mpg_mesh m, int meshloc, int64_t first, int64_t count) {
  MPG_CHECK_INIT();
  MPG_ARG(m && (meshloc == MPG_MESHLOC_ELEMENT || meshloc == MPG_MESHLOC_NODE), "mpg_mesh_set_source_window: bad mesh / location");
  const int64_t n_all = meshloc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
  MPG_ARG(first >= 0 && count >= 0 && first + count <= n_all, "mpg_mesh_set_source_window: the window must lie inside the mesh");
  const int64_t old_first = m->win_count[meshloc] >= 0 ? m->win_first[meshloc] : 0;
  store_worker_drain();
  // every handle of this mesh and location that exists already (in use or parked) moves to the new window -- after ALL of
  // them have been checked: one that references a source outside it fails the call and nothing has changed
  return cache().with_entries([&](const StoreCache<mpg_handle_s>::Map &entries) -> int {
    for (auto &kv : entries) {
      if (!kv.first.source_is(m, meshloc)) continue;
      int64_t f = 0, e = 0;
      int rc = mpg_k_source_range(kv.second, &f, &e, g_stream);
      if (rc) return rc;
      if (e > f && (f + old_first < first || e + old_first > first + count)) {
        mpg_set_error("mpg_mesh_set_source_window: a route handle of this mesh references sources [%lld, %lld), outside the window [%lld, %lld)",
                      (long long)(f + old_first), (long long)(e + old_first), (long long)first, (long long)(first + count));
        return MPG_ERR_INVALID_ARG;
      }
    }
    for (auto &kv : entries) {
      if (!kv.first.source_is(m, meshloc)) continue;
      mpg_handle_s *h = kv.second;
      h->free_tile_lists();
      h->lf_choice = 0;
      h->cf_choice = 0;
      int rc = mpg_k_rebase(h, first - old_first, count, g_stream, true);
      if (rc) return rc;
    }
    m->win_first[meshloc] = first;
    m->win_count[meshloc] = first == 0 && count == n_all ? -1 : count;   // the whole mesh: no window any more
    return MPG_SUCCESS;
  });
}

static int store_grid_entry(mpg_grid grid, int src_staggerloc, int dst_staggerloc, int regridmethod, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(grid, "mpg_regrid_store_grid: NULL argument");
  if (src_staggerloc != MPG_STAGGERLOC_CENTER || (dst_staggerloc != MPG_STAGGERLOC_EDGE1 && dst_staggerloc != MPG_STAGGERLOC_EDGE2) ||
      regridmethod != MPG_REGRIDMETHOD_BILINEAR) {
    mpg_set_error("mpg_regrid_store_grid: only bilinear CENTER -> EDGE1/EDGE2 is used by the reference (interp.F90:298,316)");
    return MPG_ERR_UNSUPPORTED;
  }
  // the inside tolerance in force is part of the handle
  return store_common(StoreKey::grid_to_grid(grid, src_staggerloc, dst_staggerloc, regridmethod, mpg_grid_inside_tol_exp()), out);
}
int mpg_regrid_store_grid(mpg_grid grid, int src_staggerloc, int dst_staggerloc, int regridmethod, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(out, "mpg_regrid_store_grid: NULL argument");
  return store_grid_entry(grid, src_staggerloc, dst_staggerloc, regridmethod, out);
}
int mpg_regrid_store_grid_begin(mpg_grid grid, int src_staggerloc, int dst_staggerloc, int regridmethod) {
  return store_grid_entry(grid, src_staggerloc, dst_staggerloc, regridmethod, nullptr);
}

// ---- Grid -> Mesh Store (k_store_to_mesh.hip) --------------------------------------------------------------------------------
// Everything that looks for "the handles whose SOURCE is this mesh" -- mpg_mesh_set_source_window, the window offset of
// mpg_handle_source_range / _unique_sources -- passes these handles by: the mesh is their destination, their sources are grid points.
static int store_to_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  return mpg_k_store_to_mesh(x.src_grid, x.src_loc, x.dst_mesh, x.dst_loc, x.method, h, s);
}

int mpg_regrid_store_to_mesh(mpg_grid src, int src_staggerloc, mpg_mesh dst, int dst_meshloc, int regridmethod, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_to_mesh: NULL argument");
  MPG_ARG(src_staggerloc >= MPG_STAGGERLOC_CENTER && src_staggerloc <= MPG_STAGGERLOC_CORNER, "mpg_regrid_store_to_mesh: unknown stagger location");
  MPG_ARG(dst_meshloc == MPG_MESHLOC_ELEMENT || dst_meshloc == MPG_MESHLOC_NODE || dst_meshloc == MPG_MESHLOC_EDGE,
          "mpg_regrid_store_to_mesh: unknown mesh location");
  MPG_ARG(dst_meshloc != MPG_MESHLOC_EDGE || dst->edge.n > 0,
          "mpg_regrid_store_to_mesh: mesh location MPG_MESHLOC_EDGE on a mesh without edges: mpg_mesh_set_edges gives it some");
  MPG_ARG(regridmethod >= 0 && regridmethod <= 2, "mpg_regrid_store_to_mesh: unknown regrid method");
  if (regridmethod == MPG_REGRIDMETHOD_CONSERVE) {
    mpg_set_error("mpg_regrid_store_to_mesh: conservative Grid -> Mesh regridding is not supported (bilinear and nearest are). "
                  "mpg_regrid_store_conserve_to_mesh is the conservative Store, with its normalisation argument.");
    return MPG_ERR_UNSUPPORTED;
  }
  if (regridmethod == MPG_REGRIDMETHOD_BILINEAR && (src->periodic & MPG_GRID_PERIODIC_I)) {
    mpg_set_error("mpg_regrid_store_to_mesh: bilinear from a periodic grid (MPG_GRID_PERIODIC_I: the i-wrap and the pole caps) is not supported; "
                  "nearest is, and mpg_regrid_store_periodic_to_mesh is the bilinear Store of such a grid, with its pole method argument");
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->geo_grid) {
    mpg_set_error("mpg_regrid_store_to_mesh: the mesh was cut to a grid (mpg_mesh_create_window): its resident cells are a window and the result "
                  "would be a partial mesh");
    return MPG_ERR_UNSUPPORTED;
  }
  const int64_t n_src = (int64_t)src->snx[src_staggerloc] * src->sny[src_staggerloc];
  const int64_t n_dst = dst_meshloc == MPG_MESHLOC_EDGE ? dst->edge.n : dst_meshloc == MPG_MESHLOC_ELEMENT ? dst->nCells : dst->nVertices;
  if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_to_mesh: %lld source points / %lld mesh points exceed int32 ids", (long long)n_src, (long long)n_dst);
    return MPG_ERR_OVERFLOW;
  }
  if (src->pts[src_staggerloc].n != n_src) {
    mpg_set_error("mpg_regrid_store_to_mesh: the grid holds no coordinates of stagger %d", src_staggerloc);
    return MPG_ERR_INVALID_ARG;
  }
  // the inside tolerance in force is part of what a bilinear handle is (as for the Grid -> Grid Store)
  return store_common(StoreKey::grid_to_mesh(src, src_staggerloc, dst, dst_meshloc, regridmethod, mpg_grid_inside_tol_exp()), out);
}

// ---- bilinear Grid -> Mesh Store of a periodic grid (k_store_periodic_to_mesh.hip) --------------------------------------------------
// A kind of its own, whatever mpg_regrid_store_to_mesh accepts one day; the two pole methods are two handles.
static int store_periodic_to_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  return mpg_k_store_periodic_to_mesh(x.src_grid, x.dst_mesh, x.dst_loc, x.pole_method, h, s);
}

int mpg_regrid_store_periodic_to_mesh(mpg_grid src, mpg_mesh dst, int dst_meshloc, int pole_method, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_periodic_to_mesh: NULL argument");
  MPG_ARG(dst_meshloc != MPG_MESHLOC_EDGE || dst->edge.n > 0,
          "mpg_regrid_store_periodic_to_mesh: unknown mesh location (MPG_MESHLOC_ELEMENT or MPG_MESHLOC_NODE; MPG_MESHLOC_EDGE needs a mesh that "
          "mpg_mesh_set_edges gave edges)");
  MPG_ARG(dst_meshloc == MPG_MESHLOC_ELEMENT || dst_meshloc == MPG_MESHLOC_NODE || dst_meshloc == MPG_MESHLOC_EDGE,
          "mpg_regrid_store_periodic_to_mesh: unknown mesh location (MPG_MESHLOC_ELEMENT or MPG_MESHLOC_NODE)");
  MPG_ARG(pole_method == MPG_POLEMETHOD_NONE || pole_method == MPG_POLEMETHOD_ALLAVG,
          "mpg_regrid_store_periodic_to_mesh: pole_method must be MPG_POLEMETHOD_NONE or MPG_POLEMETHOD_ALLAVG (NPNTAVG and TEETH are not built)");
  if (!(src->periodic & MPG_GRID_PERIODIC_I)) {
    mpg_set_error("mpg_regrid_store_periodic_to_mesh: the grid was not created with MPG_GRID_PERIODIC_I; mpg_regrid_store_to_mesh is the "
                  "Store of a regional grid");
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->geo_grid) {
    mpg_set_error("mpg_regrid_store_periodic_to_mesh: the mesh was cut to a grid (mpg_mesh_create_window): its resident cells are a window and "
                  "the result would be a partial mesh; create the whole mesh with mpg_mesh_create");
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->nx < 3 || src->ny < 2) {
    mpg_set_error("mpg_regrid_store_periodic_to_mesh: a periodic bilinear Store needs nx >= 3 and ny >= 2 CENTER points, not %d x %d", src->nx,
                  src->ny);
    return MPG_ERR_INVALID_ARG;
  }
  const int64_t n_src = (int64_t)src->nx * src->ny;
  const int64_t n_dst = dst_meshloc == MPG_MESHLOC_EDGE ? dst->edge.n : dst_meshloc == MPG_MESHLOC_ELEMENT ? dst->nCells : dst->nVertices;
  if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_periodic_to_mesh: %lld source points / %lld mesh points exceed int32 ids", (long long)n_src, (long long)n_dst);
    return MPG_ERR_OVERFLOW;
  }
  if (src->pts[MPG_STAGGERLOC_CENTER].n != n_src) {
    mpg_set_error("mpg_regrid_store_periodic_to_mesh: the grid holds no CENTER coordinates");
    return MPG_ERR_INVALID_ARG;
  }
  return store_common(StoreKey::periodic_to_mesh(src, dst, dst_meshloc, pole_method, mpg_grid_inside_tol_exp()), out);
}

// ---- conservative Grid -> Mesh Store (k_store_conserve.hip) ---------------------------------------------------------------------
static int store_conserve_to_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  return mpg_k_store_conserve_to_mesh(x.src_grid, x.dst_mesh, x.norm_type, h, s);
}

int mpg_regrid_store_conserve_to_mesh(mpg_grid src, mpg_mesh dst, int norm_type, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_conserve_to_mesh: NULL argument");
  MPG_ARG(norm_type == MPG_NORM_DSTAREA || norm_type == MPG_NORM_FRACAREA,
          "mpg_regrid_store_conserve_to_mesh: norm_type must be MPG_NORM_DSTAREA or MPG_NORM_FRACAREA");
  if (dst->geo_grid) {
    mpg_set_error("mpg_regrid_store_conserve_to_mesh: the mesh was cut to a grid (mpg_mesh_create_window): its resident cells are a window and the "
                  "result would be a partial mesh");
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->nCells > 0x7fffffffLL || (int64_t)src->nx * src->ny > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_conserve_to_mesh: %lld grid cells / %lld mesh cells exceed int32 ids", (long long)src->nx * src->ny,
                  (long long)dst->nCells);
    return MPG_ERR_OVERFLOW;
  }
  return store_common(StoreKey::conserve_to_mesh(src, dst, norm_type), out);
}

// ---- Mesh -> Mesh Store (k_store_mesh.hip) -------------------------------------------------------------------------------------
// The sources of these handles ARE the source mesh's cells (StoreKey::source_is_mesh), so everything that looks for "the handles whose
// source is this mesh" -- mpg_mesh_set_source_window, the window offset of mpg_handle_source_range / _unique_sources,
// mpg_handle_is_windowed -- finds them and treats them as it treats Mesh -> Grid handles; a window on the DESTINATION mesh does not.
// Parked entries go when either mesh is destroyed.
static int store_mesh_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  const int rc = mpg_k_store_mesh(x.src_mesh, x.dst_mesh, x.dst_loc, x.method, h, s);
  return rc ? rc : rebase_to_window(h, x.src_mesh, x.src_loc, s);
}

int mpg_regrid_store_mesh(mpg_mesh src, int src_meshloc, mpg_mesh dst, int dst_meshloc, int regridmethod, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_mesh: NULL argument");
  MPG_ARG(src_meshloc == MPG_MESHLOC_ELEMENT || src_meshloc == MPG_MESHLOC_NODE, "mpg_regrid_store_mesh: unknown source mesh location");
  MPG_ARG(dst_meshloc == MPG_MESHLOC_ELEMENT || dst_meshloc == MPG_MESHLOC_NODE, "mpg_regrid_store_mesh: unknown destination mesh location");
  MPG_ARG(regridmethod >= 0 && regridmethod <= 2, "mpg_regrid_store_mesh: unknown regrid method");
  if (regridmethod == MPG_REGRIDMETHOD_CONSERVE) {
    mpg_set_error("mpg_regrid_store_mesh: conservative Mesh -> Mesh regridding is not supported (bilinear and nearest are): the clip of "
                  "Voronoi cell against Voronoi cell is not built.  Two hops through a grid (mpg_regrid_store with MPG_REGRIDMETHOD_CONSERVE, "
                  "then mpg_regrid_store_conserve_to_mesh) are the conservative route today.  mpg_regrid_store_conserve_mesh is the "
                  "conservative Mesh -> Mesh Store, with its normalisation argument.");
    return MPG_ERR_UNSUPPORTED;
  }
  if (src_meshloc == MPG_MESHLOC_NODE) {
    mpg_set_error("mpg_regrid_store_mesh: node-located sources are not supported (the fan triangulation onto a mesh is not built); "
                  "sources are the cell centres, MPG_MESHLOC_ELEMENT -- the destination may be either location");
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->geo_grid || dst->geo_grid) {
    mpg_set_error("mpg_regrid_store_mesh: the %s mesh was cut to a grid (mpg_mesh_create_window): its resident cells are a window; "
                  "create the whole mesh with mpg_mesh_create",
                  src->geo_grid ? "source" : "destination");
    return MPG_ERR_UNSUPPORTED;
  }
  const int64_t n_dst = dst_meshloc == MPG_MESHLOC_ELEMENT ? dst->nCells : dst->nVertices;
  if (src->nCells > 0x7fffffffLL || src->nVertices > 0x7fffffffLL || n_dst > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_mesh: %lld source cells / %lld source triangles / %lld destination points exceed int32 ids",
                  (long long)src->nCells, (long long)src->nVertices, (long long)n_dst);
    return MPG_ERR_OVERFLOW;
  }
  // the line type in force is part of what a bilinear handle IS (as for the Mesh -> Grid Store)
  return store_common(StoreKey::mesh_to_mesh(src, src_meshloc, dst, dst_meshloc, regridmethod, mpg_bilinear_linetype()), out);
}

// ---- conservative Mesh -> Mesh Store (k_store_conserve_mesh.hip) -------------------------------------------------------------------
// mpg_mesh_set_source_window on the source mesh rebases these handles like every other Mesh -> Mesh handle, a window on the destination
// mesh passes them by.
static int store_conserve_mesh_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  const int rc = mpg_k_store_conserve_mesh(x.src_mesh, x.dst_mesh, x.norm_type, h, s);
  return rc ? rc : rebase_to_window(h, x.src_mesh, x.src_loc, s);
}

int mpg_regrid_store_conserve_mesh(mpg_mesh src, mpg_mesh dst, int norm_type, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_conserve_mesh: NULL argument");
  MPG_ARG(norm_type == MPG_NORM_DSTAREA || norm_type == MPG_NORM_FRACAREA,
          "mpg_regrid_store_conserve_mesh: norm_type must be MPG_NORM_DSTAREA or MPG_NORM_FRACAREA");
  if (src->geo_grid || dst->geo_grid) {
    mpg_set_error("mpg_regrid_store_conserve_mesh: the %s mesh was cut to a grid (mpg_mesh_create_window): its resident cells are a window; "
                  "create the whole mesh with mpg_mesh_create",
                  src->geo_grid ? "source" : "destination");
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->maxEdges > 12 || dst->maxEdges > 12) {
    mpg_set_error("mpg_regrid_store_conserve_mesh: maxEdges %d > 12", src->maxEdges > dst->maxEdges ? src->maxEdges : dst->maxEdges);
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->nCells > 0x7fffffffLL || dst->nCells > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_conserve_mesh: %lld source cells / %lld destination cells exceed int32 ids", (long long)src->nCells,
                  (long long)dst->nCells);
    return MPG_ERR_OVERFLOW;
  }
  return store_common(StoreKey::conserve_mesh_to_mesh(src, dst, norm_type), out);
}

// ---- Grid -> Grid Stores between two grids (k_store_to_mesh.hip, k_store_periodic_to_mesh.hip on another grid's stagger points;
// k_store_conserve_grid.hip) -------------------------------------------------------------------------------------------------------
// The bilinear and nearest searches take their destinations as a plain point set: the points of dst_staggerloc of `dst`, dnx x dny of
// them.  A handle between two different grids is marked: the wind chain must not take it for a grid's own destagger pair.
static int store_grid_to_grid_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  static const char *who = "mpg_regrid_store_grid_to_grid";
  const PointSet &dst = x.dst_grid->pts[x.dst_loc];
  const int dnx = x.dst_grid->snx[x.dst_loc], dny = x.dst_grid->sny[x.dst_loc];
  h->cross_grid = x.src_grid != x.dst_grid;
  if (x.method == MPG_REGRIDMETHOD_BILINEAR && (x.src_grid->periodic & MPG_GRID_PERIODIC_I))
    return mpg_k_store_periodic_to_points(x.src_grid, dst, (int64_t)dnx * dny, dnx, dny, x.pole_method, who, h, s);
  return mpg_k_store_to_points(x.src_grid, x.src_loc, dst, (int64_t)dnx * dny, dnx, dny, x.method, who, h, s);
}

int mpg_regrid_store_grid_to_grid(mpg_grid src, int src_staggerloc, mpg_grid dst, int dst_staggerloc, int regridmethod, int pole_method,
                                  mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_grid_to_grid: NULL argument");
  MPG_ARG(src_staggerloc >= MPG_STAGGERLOC_CENTER && src_staggerloc <= MPG_STAGGERLOC_CORNER && dst_staggerloc >= MPG_STAGGERLOC_CENTER &&
              dst_staggerloc <= MPG_STAGGERLOC_CORNER,
          "mpg_regrid_store_grid_to_grid: unknown stagger location (MPG_STAGGERLOC_CENTER, _EDGE1, _EDGE2 or _CORNER on either side)");
  MPG_ARG(regridmethod >= 0 && regridmethod <= 2,
          "mpg_regrid_store_grid_to_grid: unknown regrid method (MPG_REGRIDMETHOD_BILINEAR or MPG_REGRIDMETHOD_NEAREST_STOD)");
  MPG_ARG(pole_method == MPG_POLEMETHOD_NONE || pole_method == MPG_POLEMETHOD_ALLAVG,
          "mpg_regrid_store_grid_to_grid: pole_method must be MPG_POLEMETHOD_NONE or MPG_POLEMETHOD_ALLAVG (NPNTAVG and TEETH are not built)");
  if (regridmethod == MPG_REGRIDMETHOD_CONSERVE) {
    mpg_set_error("mpg_regrid_store_grid_to_grid: conservative regridding is not served by this call (bilinear and nearest are). "
                  "mpg_regrid_store_conserve_grid_to_grid is the conservative Store between two grids, with its normalisation argument.");
    return MPG_ERR_UNSUPPORTED;
  }
  const bool periodic_bil = regridmethod == MPG_REGRIDMETHOD_BILINEAR && (src->periodic & MPG_GRID_PERIODIC_I);
  if (periodic_bil && src_staggerloc != MPG_STAGGERLOC_CENTER) {
    mpg_set_error("mpg_regrid_store_grid_to_grid: bilinear from a grid created with MPG_GRID_PERIODIC_I takes its CENTER points only (the EDGE / "
                  "CORNER columns of a periodic grid duplicate column 0): pass MPG_STAGGERLOC_CENTER as src_staggerloc, or use "
                  "MPG_REGRIDMETHOD_NEAREST_STOD");
    return MPG_ERR_UNSUPPORTED;
  }
  const int64_t n_src = (int64_t)src->snx[src_staggerloc] * src->sny[src_staggerloc];
  const int64_t n_dst = (int64_t)dst->snx[dst_staggerloc] * dst->sny[dst_staggerloc];
  if (n_src > 0x7fffffffLL || n_dst > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_grid_to_grid: %lld source points / %lld destination points exceed int32 ids; a destination split into row "
                  "blocks stores fewer each",
                  (long long)n_src, (long long)n_dst);
    return MPG_ERR_OVERFLOW;
  }
  if (src->pts[src_staggerloc].n != n_src || dst->pts[dst_staggerloc].n != n_dst) {
    const bool s_bad = src->pts[src_staggerloc].n != n_src;
    mpg_set_error("mpg_regrid_store_grid_to_grid: the %s grid holds no coordinates of stagger %d: create the grid with them", s_bad ? "source" : "destination",
                  s_bad ? src_staggerloc : dst_staggerloc);
    return MPG_ERR_INVALID_ARG;
  }
  if (periodic_bil && (src->nx < 3 || src->ny < 2)) {
    mpg_set_error("mpg_regrid_store_grid_to_grid: a periodic bilinear Store needs nx >= 3 and ny >= 2 CENTER points, not %d x %d; "
                  "MPG_REGRIDMETHOD_NEAREST_STOD takes any grid",
                  src->nx, src->ny);
    return MPG_ERR_INVALID_ARG;
  }
  if (regridmethod == MPG_REGRIDMETHOD_BILINEAR && !periodic_bil && (src->snx[src_staggerloc] < 2 || src->sny[src_staggerloc] < 2)) {
    mpg_set_error("mpg_regrid_store_grid_to_grid: a bilinear Store needs at least 2 x 2 source points of stagger %d; MPG_REGRIDMETHOD_NEAREST_STOD "
                  "takes any grid",
                  src_staggerloc);
    return MPG_ERR_INVALID_ARG;
  }
  // the inside tolerance in force is part of what a bilinear handle is; the pole method only of a periodic source's
  return store_common(StoreKey::grid_to_other_grid(src, src_staggerloc, dst, dst_staggerloc, regridmethod, mpg_grid_inside_tol_exp(), pole_method,
                                                   (src->periodic & MPG_GRID_PERIODIC_I) != 0),
                      out);
}

static int store_conserve_grid_build(mpg_handle_s *h, const StoreCtx &x, hipStream_t s) {
  h->cross_grid = x.src_grid != x.dst_grid;
  return mpg_k_store_conserve_grid(x.src_grid, x.dst_grid, x.norm_type, h, s);
}

int mpg_regrid_store_conserve_grid_to_grid(mpg_grid src, mpg_grid dst, int norm_type, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(src && dst && out, "mpg_regrid_store_conserve_grid_to_grid: NULL argument");
  MPG_ARG(norm_type == MPG_NORM_DSTAREA || norm_type == MPG_NORM_FRACAREA,
          "mpg_regrid_store_conserve_grid_to_grid: norm_type must be MPG_NORM_DSTAREA or MPG_NORM_FRACAREA");
  for (const mpg_grid_s *g : {(const mpg_grid_s *)src, (const mpg_grid_s *)dst})
    if (g->nx < 1 || g->ny < 1 || g->pts[MPG_STAGGERLOC_CORNER].n != (int64_t)(g->nx + 1) * (g->ny + 1)) {
      mpg_set_error("mpg_regrid_store_conserve_grid_to_grid: the %s grid holds no CORNER coordinates (its cells are the quadrilaterals of four "
                    "CORNER points): create the grid with them",
                    g == src ? "source" : "destination");
      return MPG_ERR_INVALID_ARG;
    }
  if ((int64_t)(src->nx + 1) * (src->ny + 1) > 0x7fffffffLL || (int64_t)(dst->nx + 1) * (dst->ny + 1) > 0x7fffffffLL) {
    mpg_set_error("mpg_regrid_store_conserve_grid_to_grid: %lld source cells / %lld destination cells exceed int32 ids; a destination split into "
                  "row blocks stores fewer each",
                  (long long)src->nx * src->ny, (long long)dst->nx * dst->ny);
    return MPG_ERR_OVERFLOW;
  }
  return store_common(StoreKey::conserve_grid_to_grid(src, dst, norm_type), out);
}

static StoreBuildFn store_build_fn(StoreKind kind) {
  static const StoreBuildFn table[STORE_KIND_COUNT] = {store_mesh_build,             store_grid_build,      store_to_mesh_build, store_periodic_to_mesh_build,
                                                       store_conserve_to_mesh_build, store_mesh_mesh_build, store_conserve_mesh_build,
                                                       store_grid_to_grid_build,     store_conserve_grid_build};   // in StoreKind's order
  return table[kind];
}

int mpg_handle_get_dst_frac(mpg_handle h, double *frac_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && frac_host, "mpg_handle_get_dst_frac: NULL argument");
  MPG_ARG(h->dst_frac.p, "mpg_handle_get_dst_frac: the handle has no destination fraction (mpg_regrid_store_conserve_to_mesh stores one, "
                       "and so does mpg_regrid_store_conserve_mesh, and so does mpg_regrid_store_conserve_grid_to_grid)");
  MPG_HIP(hipStreamSynchronize(g_stream));
  if (h->n_dst > 0) MPG_HIP(hipMemcpy(frac_host, h->dst_frac.p, sizeof(double) * (size_t)h->n_dst, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

int mpg_handle_release(mpg_handle h) {
  if (h) cache().release(h);
  return MPG_SUCCESS;
}

// ---- Regrid ---------------------------------------------------------------------------------------
// The destination level stride of the _pitched_ calls: 0 = dense (the plane size); otherwise at least the plane, and every byte of
// nplanes planes of it must be addressable with 64-bit offsets (the kernels add k * ld to 64-bit plane bases; their buffer
// descriptors cover one plane each, so no 32-bit range grows with the stride).  -> the stride to launch with in *out
static int dst_stride(const char *who, int64_t plane, int64_t nplanes, int esz, int64_t ld, int64_t *out) {
  if (ld == 0) ld = plane;
  if (ld < plane) {
    mpg_set_error("%s: dst_level_stride %lld is below the plane size %lld", who, (long long)ld, (long long)plane);
    return MPG_ERR_INVALID_ARG;
  }
  if (ld > 0 && nplanes > 0 && nplanes > (INT64_MAX / esz) / ld) {
    mpg_set_error("%s: %lld planes of stride %lld cannot be addressed", who, (long long)nplanes, (long long)ld);
    return MPG_ERR_INVALID_ARG;
  }
  *out = ld;
  return MPG_SUCCESS;
}

int mpg_dst_level_stride(int64_t plane_points, int dst_type, int64_t *ld) {   // pure arithmetic: no mpg_init needed
  MPG_ARG(ld && plane_points >= 1, "mpg_dst_level_stride: NULL output or no points");
  MPG_ARG(dst_type >= 0 && dst_type <= 3, "mpg_dst_level_stride: dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32, optionally | MPG_TYPE_BE");
  const int64_t q = (dst_type & MPG_TYPE_F32) ? 32 : 16;   // elements per 128-byte line
  MPG_ARG(plane_points <= INT64_MAX - q, "mpg_dst_level_stride: plane too large");
  *ld = (plane_points + q - 1) / q * q;
  return MPG_SUCCESS;
}

int mpg_regrid_dev(mpg_handle h, const double *src_dev, int src_layout, int nlev, int nfields, double *dst_dev, void *hip_stream) {
  return mpg_regrid_pitched_dev(h, src_dev, src_layout, nlev, nfields, dst_dev, 0, hip_stream);
}

int mpg_regrid_pitched_dev(mpg_handle h, const double *src_dev, int src_layout, int nlev, int nfields, double *dst_dev, int64_t dst_level_stride,
                           void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h && dst_dev && (src_dev || h->n_src == 0), "mpg_regrid: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid: nlev and nfields must be >= 1");
  MPG_ARG(src_layout == MPG_LAYOUT_CELL_FAST || src_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid: bad src_layout");
  int64_t ld;
  int rc = dst_stride("mpg_regrid", h->n_dst, (int64_t)nlev * nfields, 8, dst_level_stride, &ld);
  if (rc) return rc;
  return mpg_k_apply_typed(h, src_dev, MPG_TYPE_F64, src_layout, nlev, nfields, dst_dev, MPG_TYPE_F64, 1.0, 0.0, (hipStream_t)hip_stream, FieldTab(), ld,
                           /*epi=*/false);
}

int mpg_regrid_typed_dev(mpg_handle h, const void *src_dev, int src_type, int src_layout, int nlev, int nfields, void *dst_dev,
                         int dst_type, double scale, double offset, void *hip_stream) {
  return mpg_regrid_typed_pitched_dev(h, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type, scale, offset, 0, hip_stream);
}

int mpg_regrid_typed_pitched_dev(mpg_handle h, const void *src_dev, int src_type, int src_layout, int nlev, int nfields, void *dst_dev,
                                 int dst_type, double scale, double offset, int64_t dst_level_stride, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h && dst_dev && (src_dev || h->n_src == 0), "mpg_regrid_typed: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid_typed: nlev and nfields must be >= 1");
  MPG_ARG(src_layout == MPG_LAYOUT_CELL_FAST || src_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid_typed: bad src_layout");
  MPG_ARG(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3, "mpg_regrid_typed: src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32, optionally | MPG_TYPE_BE");
  int64_t ld;
  int rc = dst_stride("mpg_regrid_typed", h->n_dst, (int64_t)nlev * nfields, (dst_type & MPG_TYPE_F32) ? 4 : 8, dst_level_stride, &ld);
  if (rc) return rc;
  return mpg_k_apply_typed(h, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type, scale, offset, (hipStream_t)hip_stream, FieldTab(), ld);
}

// ---- transpose Regrid (ESMF's transposeRoutehandle): mesh_out = A^T grid_in ---------------------------------------------
int mpg_regrid_transpose_dev(mpg_handle h, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields, void *dst_dev,
                             int dst_type, int dst_layout, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h && (dst_dev || h->n_src == 0) && (src_dev || h->n_dst == 0), "mpg_regrid_transpose: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid_transpose: nlev and nfields must be >= 1");
  MPG_ARG(dst_layout == MPG_LAYOUT_CELL_FAST || dst_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid_transpose: bad dst_layout");
  MPG_ARG(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3, "mpg_regrid_transpose: src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE) {
    mpg_set_error("mpg_regrid_transpose: big-endian values (MPG_TYPE_BE) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  int64_t ld;   // the source's level stride, checked as a destination stride is
  int rc = dst_stride("mpg_regrid_transpose: source", h->n_dst, (int64_t)nlev * nfields, (src_type & MPG_TYPE_F32) ? 4 : 8, src_level_stride, &ld);
  if (rc) return rc;
  return mpg_k_transpose(h, src_dev, src_type, ld, nlev, nfields, dst_dev, dst_type, dst_layout, (hipStream_t)hip_stream);
}

// ---- the four Regrid calls for results in mesh memory order: one set of argument checks -----------------------------------------------
struct MeshOrderCall {
  const char *name;         // as the messages give it
  int kind;                 // the handle kind the call takes
  const char *be_way;       // what follows "big-endian values (MPG_TYPE_BE) are not supported": the call that reads and writes them
  const char *other_kind;   // a handle of the other kind: the call that serves it
  const char *pole;         // a handle with pole caps
};
// ld: where the checked source level stride goes (src_level_stride as given; the checks of a destination stride).  NULL for the two
// rows calls, which have neither a stride nor a layout argument and bound nlev instead (a row's elements are counted in int).
static int check_mesh_order(const MeshOrderCall &c, mpg_handle h, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields,
                            const void *dst_dev, int dst_type, int dst_layout, int64_t *ld) {
  auto fail = [&](int rc, const char *what) {
    mpg_set_error("%s: %s", c.name, what);
    return rc;
  };
  MPG_CHECK_INIT();
  if (!(h && (dst_dev || h->n_dst == 0) && (src_dev || h->n_src == 0))) return fail(MPG_ERR_INVALID_ARG, "NULL argument");
  if (!(nlev >= 1 && nfields >= 1)) return fail(MPG_ERR_INVALID_ARG, "nlev and nfields must be >= 1");
  if (ld && dst_layout != MPG_LAYOUT_CELL_FAST && dst_layout != MPG_LAYOUT_LEV_FAST) return fail(MPG_ERR_INVALID_ARG, "bad dst_layout");
  if (!ld && nlev > (1 << 24)) return fail(MPG_ERR_INVALID_ARG, "nlev beyond 2^24");
  if (!(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3))
    return fail(MPG_ERR_INVALID_ARG, "src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE) {
    mpg_set_error("%s: big-endian values (MPG_TYPE_BE) are not supported%s", c.name, c.be_way);
    return MPG_ERR_UNSUPPORTED;
  }
  if (h->kind != c.kind) return fail(MPG_ERR_UNSUPPORTED, c.other_kind);
  if (h->n_pole > 0) return fail(MPG_ERR_UNSUPPORTED, c.pole);
  if (c.kind == MPG_KIND_FIXED && h->nnz_per_row != 1 && h->nnz_per_row != 3 && h->nnz_per_row != 4) {   // (no Store makes such a handle)
    mpg_set_error("%s: a fixed handle of %d slots is not supported (1, 3 and 4 are)", c.name, h->nnz_per_row);
    return MPG_ERR_UNSUPPORTED;
  }
  if (!ld) return MPG_SUCCESS;
  return dst_stride((std::string(c.name) + ": source").c_str(), h->n_src, (int64_t)nlev * nfields, (src_type & MPG_TYPE_F32) ? 4 : 8, src_level_stride, ld);
}

// Regrid onto a mesh in either memory order of a mesh field (k_apply_to_mesh.hip)
int mpg_regrid_to_mesh_dev(mpg_handle h, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields, void *dst_dev,
                           int dst_type, int dst_layout, double scale, double offset, void *hip_stream) {
  static const MeshOrderCall call = {"mpg_regrid_to_mesh", MPG_KIND_FIXED, "",
                                     "CSR handles (conservative, from-weights) are not supported: fixed 1-, 3- and 4-slot handles are. "
                                     "mpg_regrid_csr_to_mesh_dev serves CSR handles.",
                                     "handles with pole-cap terms (periodic Grid -> Grid) are not supported"};
  int64_t ld;
  int rc = check_mesh_order(call, h, src_dev, src_type, src_level_stride, nlev, nfields, dst_dev, dst_type, dst_layout, &ld);
  if (rc) return rc;
  return mpg_k_apply_to_mesh(h, src_dev, src_type, ld, nlev, nfields, dst_dev, dst_type, dst_layout, scale, offset, (hipStream_t)hip_stream);
}

// Regrid from [cell][lev] rows to [cell][lev] rows (k_apply_rows.hip)
int mpg_regrid_rows_dev(mpg_handle h, const void *src_dev, int src_type, int nlev, int nfields, void *dst_dev, int dst_type, double scale,
                        double offset, void *hip_stream) {
  static const MeshOrderCall call = {"mpg_regrid_rows", MPG_KIND_FIXED, "; mpg_regrid_typed_dev reads and writes them",
                                     "CSR handles (conservative, from-weights) are not supported: fixed 1-, 3- and 4-slot handles are. "
                                     "mpg_regrid_typed_dev with MPG_LAYOUT_LEV_FAST serves CSR handles from [cell][lev] rows; "
                                     "mpg_regrid_csr_rows_dev serves them from rows to rows.",
                                     "handles with pole-cap terms (periodic Grid -> Grid) are not supported; mpg_regrid_typed_dev serves them"};
  int rc = check_mesh_order(call, h, src_dev, src_type, 0, nlev, nfields, dst_dev, dst_type, 0, nullptr);
  if (rc) return rc;
  return mpg_k_apply_rows(h, src_dev, src_type, nlev, nfields, dst_dev, dst_type, scale, offset, (hipStream_t)hip_stream);
}

// Regrid of a CSR handle from [cell][lev] rows to [cell][lev] rows (k_apply_csr_rows.hip)
int mpg_regrid_csr_rows_dev(mpg_handle h, const void *src_dev, int src_type, int nlev, int nfields, void *dst_dev, int dst_type, double scale,
                            double offset, void *hip_stream) {
  static const MeshOrderCall call = {"mpg_regrid_csr_rows", MPG_KIND_CSR, "; mpg_regrid_typed_dev reads and writes them",
                                     "fixed 1-, 3- and 4-slot handles are served by mpg_regrid_rows_dev; this call takes CSR handles",
                                     "handles with pole-cap terms are not supported; mpg_regrid_typed_dev serves them"};
  int rc = check_mesh_order(call, h, src_dev, src_type, 0, nlev, nfields, dst_dev, dst_type, 0, nullptr);
  if (rc) return rc;
  return mpg_k_apply_csr_rows(h, src_dev, src_type, nlev, nfields, dst_dev, dst_type, scale, offset, (hipStream_t)hip_stream);
}

// Regrid of a CSR handle onto a mesh in either memory order (k_apply_csr_to_mesh.hip)
int mpg_regrid_csr_to_mesh_dev(mpg_handle h, const void *src_dev, int src_type, int64_t src_level_stride, int nlev, int nfields, void *dst_dev,
                               int dst_type, int dst_layout, double scale, double offset, void *hip_stream) {
  static const MeshOrderCall call = {"mpg_regrid_csr_to_mesh", MPG_KIND_CSR, "",
                                     "fixed 1-, 3- and 4-slot handles are served by mpg_regrid_to_mesh_dev; this call takes CSR handles",
                                     "handles with pole-cap terms are not supported"};
  int64_t ld;
  int rc = check_mesh_order(call, h, src_dev, src_type, src_level_stride, nlev, nfields, dst_dev, dst_type, dst_layout, &ld);
  if (rc) return rc;
  return mpg_k_apply_csr_to_mesh(h, src_dev, src_type, ld, nlev, nfields, dst_dev, dst_type, dst_layout, scale, offset, (hipStream_t)hip_stream);
}

// ---- the wind chain turned round: U / V staggers onto mesh points, one pass (k_wind_pair.hip) -----------------------------------------
// What mpg_wind_to_mesh_dev and mpg_wind_to_edges_dev, and their twins for CSR handles further down, check alike, under the caller's name: the handles, the enums, the strides (out:
// ldu / ldv in elements) and the aliases of the results r0 / r1 with each other, the sources and the angles a0 / a1.
struct WindCall {
  const char *who, *results, *angles;   // "mpg_wind_to_mesh", "ue_dev and ve_dev", "cosa_dev, sina_dev"
  bool need_angles, need_r1;            // false: both angles may be NULL together / r1 may be NULL
  bool csr;                             // the handles this call takes: CSR ones (k_wind_csr.hip) or fixed ones (k_wind_pair.hip)
  const char *twin;                     // the call that takes the other kind
};
static int wind_pair_checks(const WindCall &c, mpg_handle rh_u, mpg_handle rh_v, const double *a0, const double *a1, const void *u_dev,
                            const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *r0, void *r1,
                            int dst_type, int dst_layout, int64_t *ldu_out, int64_t *ldv_out) {
  const char *who = c.who;
  auto fail = [who](int rc, const char *what) {
    mpg_set_error("%s: %s", who, what);
    return rc;
  };
  MPG_CHECK_INIT();
  if (!(rh_u && rh_v)) return fail(MPG_ERR_INVALID_ARG, "NULL handle");
  if (!((u_dev || rh_u->n_src == 0) && (v_dev || rh_v->n_src == 0) && ((r0 && (r1 || !c.need_r1) && (!c.need_angles || (a0 && a1))) || rh_u->n_dst == 0))) return fail(MPG_ERR_INVALID_ARG, "NULL array");
  if (!c.need_angles && (a0 == nullptr) != (a1 == nullptr)) return fail(MPG_ERR_INVALID_ARG, "cosa and sina come together (both NULL: no rotation)");
  if (nlev < 1) return fail(MPG_ERR_INVALID_ARG, "nlev must be >= 1");
  if (dst_layout != MPG_LAYOUT_CELL_FAST && dst_layout != MPG_LAYOUT_LEV_FAST) return fail(MPG_ERR_INVALID_ARG, "bad dst_layout");
  if (!(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3))
    return fail(MPG_ERR_INVALID_ARG, "src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE)
    return fail(MPG_ERR_UNSUPPORTED, "big-endian values (MPG_TYPE_BE) are not supported; mpg_bswap_dev swaps an array in place before or after the call");
  for (mpg_handle h : {rh_u, rh_v}) {
    if (c.csr && h->n_pole > 0)   // (whatever its kind: the message that helps is the one about the pole terms)
      return fail(MPG_ERR_UNSUPPORTED, "handles with pole-cap terms (periodic Grid -> Grid, mpg_handle_pole_count > 0) are not supported; "
                                       "mpg_regrid_typed_dev on each handle, then the rotation, serves them");
    if (!c.csr && h->kind != MPG_KIND_FIXED) {
      mpg_set_error("%s: CSR handles (conservative, periodic, from-weights) are not supported: pairs of fixed 4-slot or 1-slot handles are. "
                    "%s serves pairs of CSR handles in one pass.", who, c.twin);
      return MPG_ERR_UNSUPPORTED;
    }
    if (c.csr && h->kind != MPG_KIND_CSR) {
      mpg_set_error("%s: fixed 1-, 3- and 4-slot handles are not supported: this call takes pairs of CSR handles. %s serves pairs of fixed "
                    "4-slot or 1-slot handles.", who, c.twin);
      return MPG_ERR_UNSUPPORTED;
    }
    if (h->n_pole > 0)
      return fail(MPG_ERR_UNSUPPORTED, "handles with pole-cap terms (periodic Grid -> Grid) are not supported; mpg_regrid_typed_dev on each handle, then "
                                       "the rotation, serves them");
  }
  if (!c.csr && (rh_u->nnz_per_row != rh_v->nnz_per_row || (rh_u->nnz_per_row != 4 && rh_u->nnz_per_row != 1))) {
    mpg_set_error("%s: handles of %d and %d slots are not supported (both 4 -- bilinear -- or both 1 -- nearest); "
                  "mpg_regrid_to_mesh_dev into float64 on each handle, then the rotation, serves any fixed pair",
                  who, rh_u->nnz_per_row, rh_v->nnz_per_row);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh_u->n_dst != rh_v->n_dst) {
    mpg_set_error("%s: the handles map onto %lld and %lld points: both must be Stores onto the same points of one mesh", who,
                  (long long)rh_u->n_dst, (long long)rh_v->n_dst);
    return MPG_ERR_INVALID_ARG;
  }
  const int es = (src_type & MPG_TYPE_F32) ? 4 : 8, ed = (dst_type & MPG_TYPE_F32) ? 4 : 8;
  // a source's level stride: 0 = dense, else at least its plane, and nlev planes of it addressable
  auto src_stride = [&](const char *arg, int64_t plane, int64_t ld, int64_t *out) {
    if (ld == 0) ld = plane;
    if (ld < plane) {
      mpg_set_error("%s: %s %lld is below the source plane of %lld points (0 = dense)", who, arg, (long long)ld, (long long)plane);
      return MPG_ERR_INVALID_ARG;
    }
    if (ld > 0 && (int64_t)nlev > (INT64_MAX / es) / ld) {
      mpg_set_error("%s: %d planes of %s %lld cannot be addressed", who, nlev, arg, (long long)ld);
      return MPG_ERR_INVALID_ARG;
    }
    *out = ld;
    return MPG_SUCCESS;
  };
  int64_t ldu = 0, ldv = 0;
  int rc;
  if ((rc = src_stride("u_level_stride", rh_u->n_src, u_level_stride, &ldu))) return rc;
  if ((rc = src_stride("v_level_stride", rh_v->n_src, v_level_stride, &ldv))) return rc;
  if (rh_u->n_dst > 0 && (int64_t)nlev > (INT64_MAX / ed) / rh_u->n_dst) return fail(MPG_ERR_INVALID_ARG, "nlev planes of n_dst results cannot be addressed");
  // neither result may alias the other, a source or the angles (a workgroup's stores would race another's loads)
  const uintptr_t nb = (uintptr_t)nlev * (uintptr_t)rh_u->n_dst * (uintptr_t)ed, na = (uintptr_t)rh_u->n_dst * sizeof(double);
  auto overlap = [](const void *p, uintptr_t np, const void *q, uintptr_t nq) {
    return p && q && (uintptr_t)p < (uintptr_t)q + nq && (uintptr_t)q < (uintptr_t)p + np;
  };
  const uintptr_t nu = (uintptr_t)nlev * (uintptr_t)ldu * (uintptr_t)es, nv = (uintptr_t)nlev * (uintptr_t)ldv * (uintptr_t)es;
  if (overlap(r0, nb, r1, nb)) {
    mpg_set_error("%s: %s alias each other: give each result its own array", who, c.results);
    return MPG_ERR_INVALID_ARG;
  }
  for (void *r : {r0, r1}) {
    if (overlap(r, nb, u_dev, nu) || overlap(r, nb, v_dev, nv))
      return fail(MPG_ERR_INVALID_ARG, "a result may not alias a source (u_dev, v_dev): give each result its own array");
    if (overlap(r, nb, a0, na) || overlap(r, nb, a1, na)) {
      mpg_set_error("%s: a result may not alias the angles (%s): give each result its own array", who, c.angles);
      return MPG_ERR_INVALID_ARG;
    }
  }
  *ldu_out = ldu;
  *ldv_out = ldv;
  return MPG_SUCCESS;
}

int mpg_wind_to_mesh_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cosa_dev, const double *sina_dev, const void *u_dev, const void *v_dev,
                         int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *ue_dev, void *ve_dev, int dst_type,
                         int dst_layout, void *hip_stream) {
  int64_t ldu, ldv;
  int rc = wind_pair_checks({"mpg_wind_to_mesh", "ue_dev and ve_dev", "cosa_dev, sina_dev", false, true, false, "mpg_wind_csr_to_mesh_dev"}, rh_u, rh_v, cosa_dev, sina_dev, u_dev, v_dev,
                            src_type, u_level_stride, v_level_stride, nlev, ue_dev, ve_dev, dst_type, dst_layout, &ldu, &ldv);
  if (rc) return rc;
  return mpg_k_wind_pair(false, rh_u, rh_v, cosa_dev, sina_dev, u_dev, v_dev, src_type, ldu, ldv, nlev, ue_dev, ve_dev, dst_type, dst_layout,
                         (hipStream_t)hip_stream);
}

// ... and onto mesh EDGES as the edge-normal wind (and the tangential one when ut_dev is given): the same checks, ONE rotation by
// phi = angleEdge - alpha whose cos / sin are required (k_wind_pair.hip: the Edges policies)
int mpg_wind_to_edges_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cn_dev, const double *sn_dev, const void *u_dev, const void *v_dev,
                          int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *un_dev, void *ut_dev, int dst_type,
                          int dst_layout, void *hip_stream) {
  int64_t ldu, ldv;
  int rc = wind_pair_checks({"mpg_wind_to_edges", "un_dev and ut_dev", "cn_dev, sn_dev", true, false, false, "mpg_wind_csr_to_edges_dev"}, rh_u, rh_v, cn_dev, sn_dev, u_dev, v_dev,
                            src_type, u_level_stride, v_level_stride, nlev, un_dev, ut_dev, dst_type, dst_layout, &ldu, &ldv);
  if (rc) return rc;
  return mpg_k_wind_pair(true, rh_u, rh_v, cn_dev, sn_dev, u_dev, v_dev, src_type, ldu, ldv, nlev, un_dev, ut_dev, dst_type, dst_layout,
                         (hipStream_t)hip_stream);
}

// ---- the same two calls for CSR handles: winds from a periodic global grid, a conservative Store, from-weights (k_wind_csr.hip) ----------
int mpg_wind_csr_to_mesh_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cosa_dev, const double *sina_dev, const void *u_dev,
                             const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *ue_dev,
                             void *ve_dev, int dst_type, int dst_layout, void *hip_stream) {
  int64_t ldu, ldv;
  int rc = wind_pair_checks({"mpg_wind_csr_to_mesh", "ue_dev and ve_dev", "cosa_dev, sina_dev", false, true, true, "mpg_wind_to_mesh_dev"}, rh_u, rh_v,
                            cosa_dev, sina_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, ue_dev, ve_dev, dst_type, dst_layout,
                            &ldu, &ldv);
  if (rc) return rc;
  return mpg_k_wind_csr(false, rh_u, rh_v, cosa_dev, sina_dev, u_dev, v_dev, src_type, ldu, ldv, nlev, ue_dev, ve_dev, dst_type, dst_layout,
                        (hipStream_t)hip_stream);
}

int mpg_wind_csr_to_edges_dev(mpg_handle rh_u, mpg_handle rh_v, const double *cn_dev, const double *sn_dev, const void *u_dev,
                              const void *v_dev, int src_type, int64_t u_level_stride, int64_t v_level_stride, int nlev, void *un_dev,
                              void *ut_dev, int dst_type, int dst_layout, void *hip_stream) {
  int64_t ldu, ldv;
  int rc = wind_pair_checks({"mpg_wind_csr_to_edges", "un_dev and ut_dev", "cn_dev, sn_dev", true, false, true, "mpg_wind_to_edges_dev"}, rh_u, rh_v,
                            cn_dev, sn_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, un_dev, ut_dev, dst_type, dst_layout,
                            &ldu, &ldv);
  if (rc) return rc;
  return mpg_k_wind_csr(true, rh_u, rh_v, cn_dev, sn_dev, u_dev, v_dev, src_type, ldu, ldv, nlev, un_dev, ut_dev, dst_type, dst_layout,
                        (hipStream_t)hip_stream);
}

// ---- a wind as a vector through one CSR handle: frames, 2 x 2 blocks, apply (k_wind_vector.hip) ------------------------------------------
// The checks are host-only text of their own (wind_vector_checks.h), so that a stand-alone program can run them.
static int wv_refused(int rc, const WvErr &e) {
  mpg_set_error("%s", e.msg);
  return rc;
}
static WvHandle wv_handle(mpg_handle rh) { return WvHandle{rh->kind == MPG_KIND_CSR, rh->n_pole, rh->n_src, rh->n_dst, rh->nnz}; }

int mpg_sphere_frames_dev(int64_t n, const double *lon_dev, const double *lat_dev, const double *c_dev, const double *s_dev,
                          double *frames_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  int rc = wv_check_frames(n, lon_dev, lat_dev, c_dev, s_dev, frames_dev, e);
  if (rc) return wv_refused(rc, e);
  return mpg_k_sphere_frames(n, lon_dev, lat_dev, c_dev, s_dev, frames_dev, (hipStream_t)hip_stream);
}

int mpg_wind_vector_weights_dev(mpg_handle rh, const double *src_frames_dev, const double *dst_frames_dev, double *m_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  WvHandle h{};
  if (rh) h = wv_handle(rh);
  bool nothing;
  int rc = wv_check_weights(rh ? &h : nullptr, src_frames_dev, dst_frames_dev, m_dev, &nothing, e);
  if (rc) return wv_refused(rc, e);
  if (nothing) return MPG_SUCCESS;   // no entries: nothing to write
  return mpg_k_wind_vector_weights(rh, src_frames_dev, dst_frames_dev, m_dev, (hipStream_t)hip_stream);
}

int mpg_wind_vector_dev(mpg_handle rh, const double *m_dev, const void *u_dev, const void *v_dev, int src_type, int64_t u_level_stride,
                        int64_t v_level_stride, int nlev, void *r0_dev, void *r1_dev, int dst_type, int dst_layout, void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  WvHandle h{};
  if (rh) h = wv_handle(rh);
  int64_t ldu, ldv;
  int rc = wv_check_apply(rh ? &h : nullptr, m_dev, u_dev, v_dev, src_type, u_level_stride, v_level_stride, nlev, r0_dev, r1_dev, dst_type, dst_layout,
                          &ldu, &ldv, e);
  if (rc) return wv_refused(rc, e);
  return mpg_k_wind_vector(rh, m_dev, u_dev, v_dev, src_type, ldu, ldv, nlev, r0_dev, r1_dev, dst_type, dst_layout, (hipStream_t)hip_stream);
}

// ---- winds from edge-normal u: the pattern of edgesOnCell, the values of (coeffs_reconstruct, frames), apply (k_wind_reconstruct.hip) ----
// The checks are host-only text of their own (wind_reconstruct_checks.h), so that a stand-alone program can run them.
static int handle_from_weights(int64_t n_src, int nx_dst, int ny_dst, int64_t nnz, const int32_t *row_host, const int32_t *col_host,
                               const double *S_host, bool force_csr, mpg_handle *out);
static WrHandle wr_handle(mpg_handle rh) { return WrHandle{wv_handle(rh), rh->max_row}; }

int mpg_reconstruct_store(int64_t nCells, int64_t nEdges, int maxEdges, const int32_t *nEdgesOnCell_host, const int32_t *edgesOnCell_host,
                          mpg_handle *out) {
  MPG_CHECK_INIT();
  WvErr e;
  int64_t nnz, max_row;
  int rc = wr_check_store(nCells, nEdges, maxEdges, nEdgesOnCell_host, edgesOnCell_host, out, &nnz, &max_row, e);
  if (rc) return wv_refused(rc, e);
  // the first nEdgesOnCell[c] slots of every cell in the file's order (the summation order), every value 1.0
  std::vector<int32_t> row((size_t)nnz + 1), col((size_t)nnz + 1);
  std::vector<double> one((size_t)nnz + 1, 1.0);
  size_t q = 0;
  for (int64_t c = 0; c < nCells; ++c)
    for (int32_t i = 0; i < nEdgesOnCell_host[c]; ++i, ++q) {
      row[q] = (int32_t)(c + 1);
      col[q] = edgesOnCell_host[c * (int64_t)maxEdges + i];
    }
  rc = handle_from_weights(nEdges, (int)nCells, 1, nnz, row.data(), col.data(), one.data(), true, out);
  if (!rc) (*out)->max_row = max_row;
  return rc;
}

int mpg_reconstruct_weights_dev(mpg_handle rh, int maxEdges, const double *coeffs_dev, const double *dst_frames_dev, double *m_dev,
                                void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  WrHandle h{};
  if (rh) h = wr_handle(rh);
  bool nothing;
  int rc = wr_check_weights(rh ? &h : nullptr, maxEdges, coeffs_dev, dst_frames_dev, m_dev, &nothing, e);
  if (rc) return wv_refused(rc, e);
  if (nothing) return MPG_SUCCESS;   // no entries: nothing to write
  return mpg_k_reconstruct_weights(rh, maxEdges, coeffs_dev, dst_frames_dev, m_dev, (hipStream_t)hip_stream);
}

int mpg_wind_reconstruct_dev(mpg_handle rh, const double *m_dev, int nout, const void *u_dev, int src_type, int src_layout, int64_t u_level_stride,
                             int nlev, void *r0_dev, void *r1_dev, void *r2_dev, int dst_type, int dst_layout, void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  WrHandle h{};
  if (rh) h = wr_handle(rh);
  int64_t ldu;
  int rc = wr_check_apply(rh ? &h : nullptr, m_dev, nout, u_dev, src_type, src_layout, u_level_stride, nlev, r0_dev, r1_dev, r2_dev, dst_type,
                          dst_layout, &ldu, e);
  if (rc) return wv_refused(rc, e);
  return mpg_k_wind_reconstruct(rh, m_dev, nout, u_dev, src_type, src_layout, ldu, nlev, r0_dev, r1_dev, r2_dev, dst_type, dst_layout,
                                (hipStream_t)hip_stream);
}

// ---- handle composition: two Regrids folded into one CSR handle (k_compose.hip) -----------------------------------------------------------
// The checks are host-only text of their own (compose_checks.h), so that a stand-alone program can run them.
static CoHandle co_handle(mpg_handle rh) { return CoHandle{rh->kind == MPG_KIND_CSR, rh->n_pole, rh->n_src, rh->n_dst, rh->nnz}; }

int mpg_handle_compose(mpg_handle outer, mpg_handle inner, mpg_handle *out) {
  MPG_CHECK_INIT();
  WvErr e;
  CoHandle a{}, b{};
  if (outer) a = co_handle(outer);
  if (inner) b = co_handle(inner);
  int rc = co_check_compose(outer ? &a : nullptr, inner ? &b : nullptr, out, e);
  if (rc) return wv_refused(rc, e);
  // Both handles are finished: a Store waits for its build before it hands its handle out, and from-weights handles are uploaded with
  // blocking copies.  The build runs on the set-up stream, as mpg_handle_get_csr's copies follow whatever produced the handle.
  mpg_handle_s *h = new mpg_handle_s();
  h->kind = MPG_KIND_CSR;
  h->method = -1;
  h->nnz_per_row = 0;
  h->n_src = inner->n_src;
  h->n_dst = outer->n_dst;
  h->nx_dst = outer->nx_dst;
  h->ny_dst = outer->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("mpg_handle_compose: hipEventCreate failed");
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_compose(outer, inner, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("mpg_handle_compose: %s", hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

int mpg_compose_weights_dev(mpg_handle composed, mpg_handle outer, mpg_handle inner, int nplanes, const double *inner_m_dev, double *m_dev,
                            void *hip_stream) {
  MPG_CHECK_INIT();
  WvErr e;
  CoHandle c{}, a{}, b{};
  if (composed) c = co_handle(composed);
  if (outer) a = co_handle(outer);
  if (inner) b = co_handle(inner);
  bool nothing;
  int rc = co_check_weights(composed ? &c : nullptr, outer ? &a : nullptr, inner ? &b : nullptr, nplanes, inner_m_dev, m_dev, &nothing, e);
  if (rc) return wv_refused(rc, e);
  if (nothing) return MPG_SUCCESS;   // no entries: nothing to write
  if (!inner_m_dev) {                // (inner has no entries: every sum is empty)
    MPG_HIP(hipMemsetAsync(m_dev, 0, sizeof(double) * (size_t)nplanes * (size_t)composed->nnz, (hipStream_t)hip_stream));
    return MPG_SUCCESS;
  }
  return mpg_k_compose_values(composed, outer, inner, nplanes, inner_m_dev, m_dev, (hipStream_t)hip_stream);
}

// ---- extrapolation: the unmapped rows of a handle filled from the nearest source points (k_extrapolate.hip) ---------------------------------
// a point set of the call: how many points, their row shape as a handle records it, and where they are
static int ex_points(const char *who, const char *role, const mpg_points *p, bool source, int64_t *n, int *nx, int *ny, const PointSet **pts) {
  if ((p->mesh != nullptr) == (p->grid != nullptr)) {
    mpg_set_error("%s: exactly one of mesh / grid must be set in the %s point set (%s are)", who, role, p->mesh ? "both" : "neither");
    return MPG_ERR_INVALID_ARG;
  }
  if (p->mesh) {
    mpg_mesh_s *m = p->mesh;
    const int loc = p->meshloc;
    if (source && loc != MPG_MESHLOC_ELEMENT) {
      mpg_set_error("%s: a source mesh is searched through its cells only (MPG_MESHLOC_ELEMENT, not location %d): "
                    "node-located sources are not served", who, loc);
      return MPG_ERR_INVALID_ARG;
    }
    if (loc != MPG_MESHLOC_ELEMENT && loc != MPG_MESHLOC_NODE && loc != MPG_MESHLOC_EDGE) {
      mpg_set_error("%s: bad mesh location %d in the %s point set", who, loc, role);
      return MPG_ERR_INVALID_ARG;
    }
    if (loc == MPG_MESHLOC_EDGE && m->edge.n == 0) {
      mpg_set_error("%s: the %s mesh has no edges: call mpg_mesh_set_edges first", who, role);
      return MPG_ERR_INVALID_ARG;
    }
    if (loc == MPG_MESHLOC_NODE && m->vwn != m->nVertices) {
      mpg_set_error("%s: the vertices of a mesh cut to a grid (mpg_mesh_create_window) are not all resident: use the whole mesh", who);
      return MPG_ERR_UNSUPPORTED;
    }
    *pts = loc == MPG_MESHLOC_EDGE ? &m->edge : loc == MPG_MESHLOC_ELEMENT ? &m->cell : &m->vert;
    *n = loc == MPG_MESHLOC_EDGE ? m->edge.n : loc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
    *nx = (int)*n;
    *ny = 1;
    return MPG_SUCCESS;
  }
  mpg_grid_s *g = p->grid;
  const int st = p->staggerloc;
  if (st < 0 || st >= 4) {
    mpg_set_error("%s: bad stagger location %d in the %s point set", who, st, role);
    return MPG_ERR_INVALID_ARG;
  }
  *nx = g->snx[st];
  *ny = g->sny[st];
  *n = (int64_t)*nx * *ny;
  *pts = &g->pts[st];
  if (g->pts[st].n != *n) {
    mpg_set_error("%s: stagger %d of the %s grid has no coordinates: create the grid with them", who, st, role);
    return MPG_ERR_INVALID_ARG;
  }
  return MPG_SUCCESS;
}

// the one body of the two entry points (below them); who: the name the messages carry
static int ex_extrapolate(const char *who, mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts,
                          const uint8_t *src_mask_dev, const uint8_t *dst_skip_dev, mpg_handle *out);

int mpg_handle_extrapolate(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts, mpg_handle *out) {
  return ex_extrapolate("mpg_handle_extrapolate", rh, src, dst, opts, nullptr, nullptr, out);
}

// ---- Store-time masks: the same fill from the UNMASKED sources only, destination rows that stay unmapped (k_extrapolate.hip, knn_mask.h)
int mpg_handle_extrapolate_masked(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts,
                                  const uint8_t *src_mask_dev, const uint8_t *dst_skip_dev, mpg_handle *out) {
  const int rc = ex_extrapolate("mpg_handle_extrapolate_masked", rh, src, dst, opts, src_mask_dev, dst_skip_dev, out);
  if (!rc && !src_mask_dev && !dst_skip_dev) (*out)->store_stats[3] = rh->n_src;   // [3] = the unmasked sources: all of them
  return rc;
}

static int ex_extrapolate(const char *who, mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_extrap_opts *opts,
                          const uint8_t *src_mask_dev, const uint8_t *dst_skip_dev, mpg_handle *out) {
  MPG_CHECK_INIT();
  if (!(rh && src && dst && opts && out)) {
    mpg_set_error("%s: NULL argument (rh, src, dst, opts and out are all mandatory)", who);
    return MPG_ERR_INVALID_ARG;
  }
  if (opts->method != MPG_EXTRAPMETHOD_NEAREST_STOD && opts->method != MPG_EXTRAPMETHOD_NEAREST_IDAVG) {
    mpg_set_error("%s: unknown method: MPG_EXTRAPMETHOD_NEAREST_STOD or MPG_EXTRAPMETHOD_NEAREST_IDAVG", who);
    return MPG_ERR_INVALID_ARG;
  }
  const bool idavg = opts->method == MPG_EXTRAPMETHOD_NEAREST_IDAVG;
  if (idavg && (opts->num_src_pnts < 1 || opts->num_src_pnts > MPG_EXTRAP_MAX_PNTS)) {
    mpg_set_error("%s: num_src_pnts = %d is outside 1..%d (MPG_EXTRAP_MAX_PNTS)", who, opts->num_src_pnts, MPG_EXTRAP_MAX_PNTS);
    return MPG_ERR_INVALID_ARG;
  }
  if (idavg && !(std::isfinite(opts->dist_exponent) && opts->dist_exponent > 0.0)) {
    mpg_set_error("%s: dist_exponent = %g must be finite and > 0 (ESMF's default is 2.0)", who, opts->dist_exponent);
    return MPG_ERR_INVALID_ARG;
  }
  int rc;
  int64_t ns = 0, nd = 0;
  int sx = 0, sy = 0, dx = 0, dy = 0;
  const PointSet *sp = nullptr, *dp = nullptr;
  if ((rc = ex_points(who, "source", src, true, &ns, &sx, &sy, &sp)) || (rc = ex_points(who, "destination", dst, false, &nd, &dx, &dy, &dp))) return rc;
  if (rh->n_pole > 0) {
    mpg_set_error("%s: the handle has pole terms (mpg_handle_pole_count > 0), which an extrapolated copy cannot carry: "
                  "store with MPG_POLEMETHOD_NONE, or fill from a non-periodic handle", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->localized) {
    mpg_set_error("%s: the handle was localized or rebased (mpg_handle_localize / mpg_handle_rebase): its indices are no "
                  "longer source ids -- extrapolate first, re-index the result", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (mpg_handle_is_windowed(rh) || (src->mesh && src->mesh->win_count[MPG_MESHLOC_ELEMENT] >= 0)) {
    mpg_set_error("%s: the source mesh carries a source window (mpg_mesh_set_source_window): the handle's indices are "
                  "window-relative -- reset the window to the whole mesh first", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_src != ns) {
    mpg_set_error("%s: the handle has n_src = %lld, the source point set has %lld points (a node-located handle has "
                  "no source set here)", who, (long long)rh->n_src, (long long)ns);
    return MPG_ERR_INVALID_ARG;
  }
  if (rh->n_dst != nd || rh->nx_dst != dx || rh->ny_dst != dy) {
    mpg_set_error("%s: the handle has n_dst = %lld (%d x %d), the destination point set has %lld points (%d x %d)", who,
                  (long long)rh->n_dst, rh->nx_dst, rh->ny_dst, (long long)nd, dx, dy);
    return MPG_ERR_INVALID_ARG;
  }
  // The search builds the source's tree (a grid's point pyramid, a mesh's site BVH): a begun Store may be building the same one on the worker.
  store_worker_drain();
  // rh is finished: a Store waits for its build before it hands its handle out.  The build runs on the set-up stream, as
  // mpg_handle_get_csr's copies follow whatever produced the handle.
  mpg_handle_s *h = new mpg_handle_s();
  h->method = rh->method;
  h->n_src = rh->n_src;
  h->n_dst = rh->n_dst;
  h->nx_dst = rh->nx_dst;
  h->ny_dst = rh->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("%s: hipEventCreate failed", who);
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_extrapolate(rh, src->mesh, src->grid, src->staggerloc, *dp, opts->method, opts->num_src_pnts, opts->dist_exponent, h, g_stream,
                         src_mask_dev, dst_skip_dev, who);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("%s: %s", who, hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

// ---- nearest destination to source: every source onto its nearest destination point, a CSR handle built by scattering (k_store_dtos.hip) ------
// a point set of the call: how many points, their row shape as a handle records it, and where they are
static int dtos_points(const char *who, const char *role, const mpg_points *p, bool source, int64_t *n, int *nx, int *ny, const PointSet **pts) {
  if ((p->mesh != nullptr) == (p->grid != nullptr)) {
    mpg_set_error("%s: exactly one of mesh / grid must be set in the %s point set (%s are)", who, role, p->mesh ? "both" : "neither");
    return MPG_ERR_INVALID_ARG;
  }
  if (p->mesh) {
    mpg_mesh_s *m = p->mesh;
    const int loc = p->meshloc;
    if (loc != MPG_MESHLOC_ELEMENT && loc != MPG_MESHLOC_NODE && loc != MPG_MESHLOC_EDGE) {
      mpg_set_error("%s: bad mesh location %d in the %s point set", who, loc, role);
      return MPG_ERR_INVALID_ARG;
    }
    if (!source && loc != MPG_MESHLOC_ELEMENT) {
      mpg_set_error("%s: a destination mesh is searched through its cells only (MPG_MESHLOC_ELEMENT, not location %d): no tree is built over "
                    "vertices or edges -- aggregate onto the cells, or onto a grid stagger", who, loc);
      return MPG_ERR_UNSUPPORTED;
    }
    if (m->geo_grid) {
      mpg_set_error("%s: the %s mesh was cut to a grid (mpg_mesh_create_window): its resident points are a window; use the whole mesh "
                    "(mpg_mesh_create)", who, role);
      return MPG_ERR_UNSUPPORTED;
    }
    if (!source && m->win_count[MPG_MESHLOC_ELEMENT] >= 0) {
      mpg_set_error("%s: the destination mesh carries a source window (mpg_mesh_set_source_window): reset the window to the whole mesh "
                    "first", who);
      return MPG_ERR_UNSUPPORTED;
    }
    if (loc == MPG_MESHLOC_EDGE && m->edge.n == 0) {
      mpg_set_error("%s: the %s mesh has no edges: call mpg_mesh_set_edges first", who, role);
      return MPG_ERR_INVALID_ARG;
    }
    *pts = loc == MPG_MESHLOC_EDGE ? &m->edge : loc == MPG_MESHLOC_ELEMENT ? &m->cell : &m->vert;
    *n = loc == MPG_MESHLOC_EDGE ? m->edge.n : loc == MPG_MESHLOC_ELEMENT ? m->nCells : m->nVertices;
    if (*n > 0x7fffffffll) {
      mpg_set_error("%s: the %s point set has %lld points, more than int32 ids hold", who, role, (long long)*n);
      return MPG_ERR_OVERFLOW;
    }
    *nx = (int)*n;
    *ny = 1;
    return MPG_SUCCESS;
  }
  mpg_grid_s *g = p->grid;
  const int st = p->staggerloc;
  if (st < 0 || st >= 4) {
    mpg_set_error("%s: bad stagger location %d in the %s point set", who, st, role);
    return MPG_ERR_INVALID_ARG;
  }
  *nx = g->snx[st];
  *ny = g->sny[st];
  *n = (int64_t)*nx * *ny;
  *pts = &g->pts[st];
  if (g->pts[st].n != *n) {
    mpg_set_error("%s: stagger %d of the %s grid has no coordinates: create the grid with them", who, st, role);
    return MPG_ERR_INVALID_ARG;
  }
  if (*n > 0x7fffffffll) {
    mpg_set_error("%s: the %s point set has %lld points, more than int32 ids hold", who, role, (long long)*n);
    return MPG_ERR_OVERFLOW;
  }
  return MPG_SUCCESS;
}

int mpg_regrid_store_nearest_dtos(const mpg_points *src, const mpg_points *dst, int norm, const uint8_t *src_mask_dev,
                                  const uint8_t *dst_mask_dev, mpg_handle *out) {
  const char *who = "mpg_regrid_store_nearest_dtos";
  MPG_CHECK_INIT();
  if (!(src && dst && out)) {
    mpg_set_error("%s: NULL argument (src, dst and out are all mandatory)", who);
    return MPG_ERR_INVALID_ARG;
  }
  if (norm != MPG_DTOS_SUM && norm != MPG_DTOS_MEAN) {
    mpg_set_error("%s: unknown norm %d: MPG_DTOS_SUM or MPG_DTOS_MEAN", who, norm);
    return MPG_ERR_INVALID_ARG;
  }
  int rc;
  int64_t ns = 0, nd = 0;
  int sx = 0, sy = 0, dx = 0, dy = 0;
  const PointSet *sp = nullptr, *dp = nullptr;
  if ((rc = dtos_points(who, "source", src, true, &ns, &sx, &sy, &sp)) || (rc = dtos_points(who, "destination", dst, false, &nd, &dx, &dy, &dp))) return rc;
  // The search builds the destination's tree (a grid's point pyramid, a mesh's site BVH): a begun Store may be building the same one on the worker.
  store_worker_drain();
  mpg_handle_s *h = new mpg_handle_s();
  h->method = MPG_REGRIDMETHOD_NEAREST_DTOS;
  h->n_src = ns;
  h->n_dst = nd;
  h->nx_dst = dx;
  h->ny_dst = dy;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("%s: hipEventCreate failed", who);
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_store_dtos(*sp, ns, src->mesh != nullptr, dst->mesh, dst->grid, dst->staggerloc, norm, src_mask_dev, dst_mask_dev, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("%s: %s", who, hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

int mpg_handle_get_src_nearest(mpg_handle h, int32_t *nearest_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && nearest_host, "mpg_handle_get_src_nearest: NULL argument");
  MPG_ARG(h->has_src_nearest, "mpg_handle_get_src_nearest: the handle keeps no nearest[] (mpg_regrid_store_nearest_dtos stores one; no other "
                              "call does)");
  if (h->n_src > 0) {
    MPG_HIP(hipStreamSynchronize(g_stream));
    MPG_HIP(hipMemcpy(nearest_host, h->src_nearest.p, sizeof(int32_t) * (size_t)h->n_src, hipMemcpyDeviceToHost));
  }
  return MPG_SUCCESS;
}

// ---- Store-time masks on a handle's pattern (k_handle_mask.hip): no geometry, every Store and every consumer served at once ----------------
int mpg_handle_mask(mpg_handle rh, const mpg_store_mask_opts *opts, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(rh && opts && out, "mpg_handle_mask: NULL argument (rh, opts and out are all mandatory)");
  MPG_ARG(opts->rule == MPG_MASKRULE_AUTO || opts->rule == MPG_MASKRULE_ROW || opts->rule == MPG_MASKRULE_ENTRY,
          "mpg_handle_mask: unknown rule: MPG_MASKRULE_AUTO, MPG_MASKRULE_ROW or MPG_MASKRULE_ENTRY");
  int rule = opts->rule;
  if (rule == MPG_MASKRULE_AUTO) {
    if (rh->method == MPG_REGRIDMETHOD_BILINEAR || rh->method == MPG_REGRIDMETHOD_NEAREST_STOD || rh->method == MPG_REGRIDMETHOD_PATCH) rule = MPG_MASKRULE_ROW;
    else if (rh->method == MPG_REGRIDMETHOD_CONSERVE) rule = MPG_MASKRULE_ENTRY;
    else if (rh->method == MPG_REGRIDMETHOD_NEAREST_DTOS) {
      mpg_set_error("mpg_handle_mask: MPG_MASKRULE_AUTO does not serve a nearest-destination-to-source handle: a destination masked afterwards "
                    "would not re-route its sources -- pass the masks to mpg_regrid_store_nearest_dtos (src_mask_dev, dst_mask_dev), or name "
                    "MPG_MASKRULE_ROW / MPG_MASKRULE_ENTRY");
      return MPG_ERR_UNSUPPORTED;
    } else {
      mpg_set_error("mpg_handle_mask: MPG_MASKRULE_AUTO follows the handle's regrid method, and this handle records none (from weights, "
                    "composed, reconstruct): pass MPG_MASKRULE_ROW or MPG_MASKRULE_ENTRY");
      return MPG_ERR_INVALID_ARG;
    }
  }
  const bool entry = rule == MPG_MASKRULE_ENTRY;
  if (entry) MPG_ARG(opts->norm_type == MPG_NORM_DSTAREA || opts->norm_type == MPG_NORM_FRACAREA,
                     "mpg_handle_mask: unknown norm_type: MPG_NORM_DSTAREA or MPG_NORM_FRACAREA, the one the Store was called with");
  if (rh->n_pole > 0) {
    mpg_set_error("mpg_handle_mask: the handle has pole terms (mpg_handle_pole_count > 0), which a masked copy cannot carry: store with "
                  "MPG_POLEMETHOD_NONE");
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->localized) {
    mpg_set_error("mpg_handle_mask: the handle was localized or rebased (mpg_handle_localize / mpg_handle_rebase): its indices are no longer "
                  "source ids -- mask first, re-index the result");
    return MPG_ERR_UNSUPPORTED;
  }
  if (mpg_handle_is_windowed(rh)) {
    mpg_set_error("mpg_handle_mask: the source mesh carries a source window (mpg_mesh_set_source_window): the handle's indices are "
                  "window-relative -- reset the window to the whole mesh first");
    return MPG_ERR_UNSUPPORTED;
  }
  if (entry && rh->kind != MPG_KIND_CSR) {
    mpg_set_error("mpg_handle_mask: MPG_MASKRULE_ENTRY removes entries, which the slots of a fixed handle cannot express: "
                  "mpg_handle_get_weights, then mpg_handle_from_weights, makes a CSR handle of it (or use MPG_MASKRULE_ROW)");
    return MPG_ERR_UNSUPPORTED;
  }
  // rh is finished (a Store waits for its build before it hands its handle out); a begun Store may still allocate on the worker
  store_worker_drain();
  mpg_handle_s *h = new mpg_handle_s();
  h->method = rh->method;
  h->n_src = rh->n_src;
  h->n_dst = rh->n_dst;
  h->nx_dst = rh->nx_dst;
  h->ny_dst = rh->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("mpg_handle_mask: hipEventCreate failed");
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  int rc = mpg_k_handle_mask(rh, opts->src_mask_dev, opts->dst_mask_dev, entry, opts->norm_type, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("mpg_handle_mask: %s", hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

// ---- patch regridding: a fixed bilinear handle turned into the CSR handle of second-degree patch recovery (k_patch.hip, patch.h) ------------
int mpg_handle_patch(mpg_handle rh, const mpg_points *src, const mpg_points *dst, mpg_handle *out) {
  const char *who = "mpg_handle_patch";
  MPG_CHECK_INIT();
  if (!(rh && src && dst && out)) {
    mpg_set_error("%s: NULL argument (rh, src, dst and out are all mandatory)", who);
    return MPG_ERR_INVALID_ARG;
  }
  int rc;
  int64_t ns = 0, nd = 0;
  int sx = 0, sy = 0, dx = 0, dy = 0;
  const PointSet *sp = nullptr, *dp = nullptr;
  if ((rc = ex_points(who, "source", src, true, &ns, &sx, &sy, &sp)) || (rc = ex_points(who, "destination", dst, false, &nd, &dx, &dy, &dp))) return rc;
  if (rh->method != MPG_REGRIDMETHOD_BILINEAR) {
    mpg_set_error("%s: the handle's method is %d, not MPG_REGRIDMETHOD_BILINEAR: the patch rule blends the polynomials of a bilinear "
                  "row's nodes -- store bilinear, then patch", who, rh->method);
    return MPG_ERR_INVALID_ARG;
  }
  if (rh->kind != MPG_KIND_FIXED || (rh->nnz_per_row != 3 && rh->nnz_per_row != 4) || !rh->w.p) {
    mpg_set_error("%s: a %s handle is not served: the rule reads the 3 or 4 slots of a fixed bilinear handle (mpg_regrid_store, _store_mesh, "
                  "_store_to_mesh, _store_grid) -- patch first, then mpg_handle_mask / mpg_handle_extrapolate", who,
                  rh->kind == MPG_KIND_CSR ? "CSR" : "1-slot");
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->mesh && src->mesh->geo_grid) {
    mpg_set_error("%s: the source mesh was cut to a grid (mpg_mesh_create_window): the patches need every cell's vertices and triangles "
                  "-- use the whole mesh (mpg_mesh_create)", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_pole > 0) {
    mpg_set_error("%s: the handle has pole terms (mpg_handle_pole_count > 0), which a patch handle cannot carry: store with "
                  "MPG_POLEMETHOD_NONE, or patch a non-periodic handle", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->localized) {
    mpg_set_error("%s: the handle was localized or rebased (mpg_handle_localize / mpg_handle_rebase): its indices are no "
                  "longer source ids -- patch first, re-index the result", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (mpg_handle_is_windowed(rh) || (src->mesh && src->mesh->win_count[MPG_MESHLOC_ELEMENT] >= 0)) {
    mpg_set_error("%s: the source mesh carries a source window (mpg_mesh_set_source_window): the handle's indices are "
                  "window-relative -- reset the window to the whole mesh first", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->grid && (src->grid->periodic & MPG_GRID_PERIODIC_I)) {
    mpg_set_error("%s: a source grid with MPG_GRID_PERIODIC_I is not served (the 3 x 3 windows do not wrap in i and know no pole): "
                  "create the grid without the flag, or regrid bilinearly", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_src != ns) {
    mpg_set_error("%s: the handle has n_src = %lld, the source point set has %lld points (a node-located handle has "
                  "no source set here)", who, (long long)rh->n_src, (long long)ns);
    return MPG_ERR_INVALID_ARG;
  }
  if (rh->n_dst != nd || rh->nx_dst != dx || rh->ny_dst != dy) {
    mpg_set_error("%s: the handle has n_dst = %lld (%d x %d), the destination point set has %lld points (%d x %d)", who,
                  (long long)rh->n_dst, rh->nx_dst, rh->ny_dst, (long long)nd, dx, dy);
    return MPG_ERR_INVALID_ARG;
  }
  if (ns > 0x7fffffffLL) {
    mpg_set_error("%s: %lld source points are beyond int32 ids", who, (long long)ns);
    return MPG_ERR_OVERFLOW;
  }
  PtSrc ps;
  ps.x = sp->x.p; ps.y = sp->y.p; ps.z = sp->z.p;
  ps.voc = nullptr; ps.tri = nullptr; ps.maxEdges = 0; ps.nV = 0; ps.snx = sx; ps.sny = sy;
  if (src->mesh) {
    ps.voc = src->mesh->voc.p; ps.tri = src->mesh->tri.p; ps.maxEdges = src->mesh->maxEdges; ps.nV = src->mesh->nVertices;
  }
  // rh is finished (a Store waits for its build before it hands its handle out); a begun Store may still allocate on the worker
  store_worker_drain();
  mpg_handle_s *h = new mpg_handle_s();
  h->method = MPG_REGRIDMETHOD_PATCH;
  h->n_src = rh->n_src;
  h->n_dst = rh->n_dst;
  h->nx_dst = rh->nx_dst;
  h->ny_dst = rh->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("%s: hipEventCreate failed", who);
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_patch(rh, ps, *dp, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("%s: %s", who, hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

// ---- second-order conservative regridding: a first-order conservative CSR handle turned into the CSR handle of a linear reconstruction
// inside every source cell (k_conserve2nd.hip, conserve2nd.h) ---------------------------------------------------------------------------------
int mpg_handle_conserve2nd(mpg_handle rh, const mpg_points *src, const mpg_points *dst, const mpg_conserve2nd_opts *opts, mpg_handle *out) {
  const char *who = "mpg_handle_conserve2nd";
  MPG_CHECK_INIT();
  if (!(rh && src && dst && opts && out)) {
    mpg_set_error("%s: NULL argument (rh, src, dst, opts and out are all mandatory)", who);
    return MPG_ERR_INVALID_ARG;
  }
  int rc;
  int64_t ns = 0, nd = 0;
  int sx = 0, sy = 0, dx = 0, dy = 0;
  const PointSet *sp = nullptr, *dp = nullptr;
  if ((rc = ex_points(who, "source", src, true, &ns, &sx, &sy, &sp)) || (rc = ex_points(who, "destination", dst, false, &nd, &dx, &dy, &dp))) return rc;
  if (dst->mesh && dst->meshloc != MPG_MESHLOC_ELEMENT) {
    mpg_set_error("%s: the destination mesh takes part with its cells (MPG_MESHLOC_ELEMENT, not location %d): conservative handles map "
                  "cells to cells", who, dst->meshloc);
    return MPG_ERR_INVALID_ARG;
  }
  if ((src->grid && src->staggerloc != MPG_STAGGERLOC_CENTER) || (dst->grid && dst->staggerloc != MPG_STAGGERLOC_CENTER)) {
    mpg_set_error("%s: a grid takes part with its cells (MPG_STAGGERLOC_CENTER, not stagger %d): conservative handles map cells to cells", who,
                  src->grid && src->staggerloc != MPG_STAGGERLOC_CENTER ? src->staggerloc : dst->staggerloc);
    return MPG_ERR_INVALID_ARG;
  }
  if (opts->norm_type != MPG_NORM_DSTAREA && opts->norm_type != MPG_NORM_FRACAREA) {
    mpg_set_error("%s: unknown norm_type %d: MPG_NORM_DSTAREA or MPG_NORM_FRACAREA, the one the Store was called with", who, opts->norm_type);
    return MPG_ERR_INVALID_ARG;
  }
  if (rh->method != MPG_REGRIDMETHOD_CONSERVE) {
    mpg_set_error("%s: the handle's method is %d, not MPG_REGRIDMETHOD_CONSERVE: the rule re-clips the stored pairs of a first-order "
                  "conservative handle -- store conservatively, then convert", who, rh->method);
    return MPG_ERR_INVALID_ARG;
  }
  for (int side = 0; side < 2; ++side) {
    const mpg_grid_s *g = side ? dst->grid : src->grid;
    if (!g) continue;
    const int64_t want = (int64_t)(g->nx + 1) * (g->ny + 1);
    if (g->pts[MPG_STAGGERLOC_CORNER].n != want) {
      mpg_set_error("%s: the %s grid has no CORNER coordinates (%lld points, %lld expected): its cells are the quadrilaterals of the CORNER "
                    "stagger -- create the grid with them", who, side ? "destination" : "source", (long long)g->pts[MPG_STAGGERLOC_CORNER].n,
                    (long long)want);
      return MPG_ERR_INVALID_ARG;
    }
  }
  if (rh->kind != MPG_KIND_CSR) {
    mpg_set_error("%s: a fixed handle is not served: the rule reads the rows of a conservative CSR handle (mpg_regrid_store with "
                  "MPG_REGRIDMETHOD_CONSERVE, mpg_regrid_store_conserve_to_mesh, mpg_regrid_store_conserve_mesh)", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_pole > 0) {
    mpg_set_error("%s: the handle has pole terms (mpg_handle_pole_count > 0), which a second-order handle cannot carry: store with "
                  "MPG_POLEMETHOD_NONE", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->localized) {
    mpg_set_error("%s: the handle was localized or rebased (mpg_handle_localize / mpg_handle_rebase): its indices are no "
                  "longer source ids -- convert first, re-index the result", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (mpg_handle_is_windowed(rh) || (src->mesh && src->mesh->win_count[MPG_MESHLOC_ELEMENT] >= 0)) {
    mpg_set_error("%s: the source mesh carries a source window (mpg_mesh_set_source_window): the handle's indices are "
                  "window-relative -- reset the window to the whole mesh first", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if ((src->mesh && src->mesh->geo_grid) || (dst->mesh && dst->mesh->geo_grid)) {
    mpg_set_error("%s: the %s mesh was cut to a grid (mpg_mesh_create_window): the re-clip and the rings need every cell's vertices and "
                  "triangles -- use the whole mesh (mpg_mesh_create)", who, src->mesh && src->mesh->geo_grid ? "source" : "destination");
    return MPG_ERR_UNSUPPORTED;
  }
  if ((src->mesh && src->mesh->maxEdges > 12) || (dst->mesh && dst->mesh->maxEdges > 12)) {
    mpg_set_error("%s: maxEdges %d > 12: the clip holds cells of at most 12 vertices -- split the larger cells", who,
                  std::max(src->mesh ? src->mesh->maxEdges : 0, dst->mesh ? dst->mesh->maxEdges : 0));
    return MPG_ERR_UNSUPPORTED;
  }
  if (src->grid && (src->grid->periodic & MPG_GRID_PERIODIC_I)) {
    mpg_set_error("%s: a source grid with MPG_GRID_PERIODIC_I is not served (the 3 x 3 rings do not wrap in i and know no pole): "
                  "create the grid without the flag, or stay first order", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_src != ns) {
    mpg_set_error("%s: the handle has n_src = %lld, the source point set has %lld cells", who, (long long)rh->n_src, (long long)ns);
    return MPG_ERR_INVALID_ARG;
  }
  if (rh->n_dst != nd || rh->nx_dst != dx || rh->ny_dst != dy) {
    mpg_set_error("%s: the handle has n_dst = %lld (%d x %d), the destination point set has %lld cells (%d x %d)", who,
                  (long long)rh->n_dst, rh->nx_dst, rh->ny_dst, (long long)nd, dx, dy);
    return MPG_ERR_INVALID_ARG;
  }
  if (ns > 0x7fffffffLL) {
    mpg_set_error("%s: %lld source cells are beyond int32 ids", who, (long long)ns);
    return MPG_ERR_OVERFLOW;
  }
  PtSrc ps;
  ps.x = sp->x.p; ps.y = sp->y.p; ps.z = sp->z.p;
  ps.voc = nullptr; ps.tri = nullptr; ps.maxEdges = 0; ps.nV = 0; ps.snx = sx; ps.sny = sy;
  if (src->mesh) {
    ps.voc = src->mesh->voc.p; ps.tri = src->mesh->tri.p; ps.maxEdges = src->mesh->maxEdges; ps.nV = src->mesh->nVertices;
  }
  // rh is finished (a Store waits for its build before it hands its handle out); a begun Store may still allocate on the worker.  The
  // build runs on the set-up stream, after whatever produced rh
  store_worker_drain();
  mpg_handle_s *h = new mpg_handle_s();
  h->method = MPG_REGRIDMETHOD_CONSERVE_2ND;
  h->n_src = rh->n_src;
  h->n_dst = rh->n_dst;
  h->nx_dst = rh->nx_dst;
  h->ny_dst = rh->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("%s: hipEventCreate failed", who);
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_conserve2nd(rh, src->mesh, src->grid, dst->mesh, dst->grid, ps, opts->norm_type, opts->src_mask_dev, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("%s: %s", who, hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

// ---- creep-fill extrapolation: the unmapped rows of a handle filled level by level from their neighbours' rows (k_creep.hip, creep.h) -------
int mpg_handle_creep(mpg_handle rh, const mpg_points *dst, const mpg_creep_opts *opts, mpg_handle *out) {
  const char *who = "mpg_handle_creep";
  MPG_CHECK_INIT();
  if (!(rh && dst && opts && out)) {
    mpg_set_error("%s: NULL argument (rh, dst, opts and out are all mandatory)", who);
    return MPG_ERR_INVALID_ARG;
  }
  int rc;
  int64_t nd = 0;
  int dx = 0, dy = 0;
  const PointSet *dp = nullptr;
  if ((rc = ex_points(who, "destination", dst, false, &nd, &dx, &dy, &dp))) return rc;   // (mpg_handle_extrapolate's point-set rules)
  if (opts->num_levels < 1) {
    mpg_set_error("%s: num_levels = %d must be >= 1 (ESMF's extrapNumLevels; MPG_CREEP_ALL_LEVELS fills until no row is reached any more)", who,
                  opts->num_levels);
    return MPG_ERR_INVALID_ARG;
  }
  // the handle first (a handle with pole terms only ever meets a periodic destination), then the destination
  if (rh->n_pole > 0) {
    mpg_set_error("%s: the handle has pole terms (mpg_handle_pole_count > 0), which a crept copy cannot carry: store with "
                  "MPG_POLEMETHOD_NONE, or creep a non-periodic handle", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->localized || mpg_handle_is_windowed(rh)) {
    mpg_set_error("%s: the handle was localized or rebased (mpg_handle_localize / mpg_handle_rebase), or its mesh carries a source window "
                  "(mpg_mesh_set_source_window): its indices are no longer source ids -- creep first, re-index the result", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->mesh && dst->meshloc != MPG_MESHLOC_ELEMENT) {
    mpg_set_error("%s: a destination mesh is crept over its cells only (MPG_MESHLOC_ELEMENT, not location %d): no ring is defined on "
                  "vertices or edges -- fill those with mpg_handle_extrapolate", who, dst->meshloc);
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->mesh && dst->mesh->geo_grid) {
    mpg_set_error("%s: the destination mesh was cut to a grid (mpg_mesh_create_window): the rings need every cell's vertices and triangles "
                  "-- use the whole mesh (mpg_mesh_create)", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->mesh && dst->mesh->maxEdges > CR_MAX_EDGES) {
    mpg_set_error("%s: maxEdges %d > %d: a cell's ring holds at most %d neighbours -- split the larger cells", who, dst->mesh->maxEdges,
                  CR_MAX_EDGES, CR_MAX_NB);
    return MPG_ERR_UNSUPPORTED;
  }
  if (dst->grid && (dst->grid->periodic & MPG_GRID_PERIODIC_I)) {
    mpg_set_error("%s: a destination grid with MPG_GRID_PERIODIC_I is not served (the neighbourhoods do not wrap in i: the seam would be a "
                  "wall): create the grid without the flag, or fill with mpg_handle_extrapolate", who);
    return MPG_ERR_UNSUPPORTED;
  }
  if (rh->n_dst != nd || rh->nx_dst != dx || rh->ny_dst != dy) {
    mpg_set_error("%s: the handle has n_dst = %lld (%d x %d), the destination point set has %lld points (%d x %d)", who,
                  (long long)rh->n_dst, rh->nx_dst, rh->ny_dst, (long long)nd, dx, dy);
    return MPG_ERR_INVALID_ARG;
  }
  if (nd > 0x7ffffffeLL) {
    mpg_set_error("%s: %lld destination points are beyond int32 ids", who, (long long)nd);
    return MPG_ERR_OVERFLOW;
  }
  PtSrc pd;   // the destination's connectivity alone: no coordinates are read
  pd.x = pd.y = pd.z = nullptr;
  pd.voc = nullptr; pd.tri = nullptr; pd.maxEdges = 0; pd.nV = 0; pd.snx = dx; pd.sny = dy;
  if (dst->mesh) {
    pd.voc = dst->mesh->voc.p; pd.tri = dst->mesh->tri.p; pd.maxEdges = dst->mesh->maxEdges; pd.nV = dst->mesh->nVertices;
  }
  // rh is finished (a Store waits for its build before it hands its handle out); a begun Store may still allocate on the worker.  The
  // build runs on the set-up stream, after whatever produced rh
  store_worker_drain();
  mpg_handle_s *h = new mpg_handle_s();
  h->method = rh->method;
  h->n_src = rh->n_src;
  h->n_dst = rh->n_dst;
  h->nx_dst = rh->nx_dst;
  h->ny_dst = rh->ny_dst;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    mpg_set_error("%s: hipEventCreate failed", who);
    handle_free(h);
    return MPG_ERR_HIP;
  }
  (void)hipEventRecord(e0, g_stream);
  rc = mpg_k_creep(rh, pd, opts->num_levels, opts->dst_skip_dev, h, g_stream);
  if (!rc) {
    hipError_t he = hipEventRecord(e1, g_stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    if (he == hipSuccess) he = hipEventElapsedTime(&h->store_ms, e0, e1);
    if (he != hipSuccess) {
      mpg_set_error("%s: %s", who, hipGetErrorString(he));
      rc = MPG_ERR_HIP;
    }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) {
    (void)hipStreamSynchronize(g_stream);   // nothing of the failed build still runs on arrays that go now
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

// ---- masked Regrid: missing sources skipped, the valid ones renormalised, fill elsewhere (k_apply_masked.hip) --------------
int mpg_regrid_masked_dev(mpg_handle h, const void *src_dev, int src_type, int src_layout, int nlev, int nfields, void *dst_dev, int dst_type,
                          int64_t dst_level_stride, const mpg_mask_opts *opts, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_regrid_masked: NULL handle");
  MPG_ARG(opts, "mpg_regrid_masked: NULL options");
  MPG_ARG(dst_dev && (src_dev || h->n_src == 0), "mpg_regrid_masked: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid_masked: nlev and nfields must be >= 1");
  MPG_ARG(src_layout == MPG_LAYOUT_CELL_FAST || src_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid_masked: bad src_layout");
  MPG_ARG(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3, "mpg_regrid_masked: src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((src_type | dst_type) & MPG_TYPE_BE) {
    mpg_set_error("mpg_regrid_masked: big-endian values (MPG_TYPE_BE) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  if (h->n_pole > 0) {
    mpg_set_error("mpg_regrid_masked: handles with pole-cap terms (periodic Grid -> Grid) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG((opts->flags & ~(MPG_MISSING_NAN | MPG_MISSING_VALUE)) == 0, "mpg_regrid_masked: unknown flag bits");
  MPG_ARG(opts->min_valid_frac >= 0.0 && opts->min_valid_frac <= 1.0, "mpg_regrid_masked: min_valid_frac must lie in [0, 1]");   // (false for NaN)
  MPG_ARG(!(opts->flags & MPG_MISSING_VALUE) || opts->missing_value == opts->missing_value, "mpg_regrid_masked: MPG_MISSING_VALUE with a NaN missing_value (use MPG_MISSING_NAN)");
  int64_t ld;
  int rc = dst_stride("mpg_regrid_masked", h->n_dst, (int64_t)nlev * nfields, (dst_type & MPG_TYPE_F32) ? 4 : 8, dst_level_stride, &ld);
  if (rc) return rc;
  return mpg_k_apply_masked(h, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type, ld, opts, (hipStream_t)hip_stream);
}

// ---- its adjoint: the scaled gradient h into the caller's workspace, then the transposed gather with the select (k_transpose_masked.hip) ----
int mpg_regrid_masked_transpose_dev(mpg_handle h, const void *g_dev, int g_type, int64_t g_level_stride, const void *src_dev, int src_type,
                                    int src_layout, int nlev, int nfields, void *dst_dev, int dst_type, const mpg_mask_opts *opts, double *work_dev,
                                    void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_regrid_masked_transpose: NULL handle");
  MPG_ARG(opts, "mpg_regrid_masked_transpose: NULL options");
  MPG_ARG(g_dev && src_dev && dst_dev && work_dev, "mpg_regrid_masked_transpose: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid_masked_transpose: nlev and nfields must be >= 1");
  MPG_ARG(src_layout == MPG_LAYOUT_CELL_FAST || src_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid_masked_transpose: bad src_layout");
  MPG_ARG(g_type >= 0 && g_type <= 3 && src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3,
          "mpg_regrid_masked_transpose: g_type / src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if ((g_type | src_type | dst_type) & MPG_TYPE_BE) {
    mpg_set_error("mpg_regrid_masked_transpose: big-endian values (MPG_TYPE_BE) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  if (h->n_pole > 0) {
    mpg_set_error("mpg_regrid_masked_transpose: handles with pole-cap terms (periodic Grid -> Grid) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG((opts->flags & ~(MPG_MISSING_NAN | MPG_MISSING_VALUE)) == 0, "mpg_regrid_masked_transpose: unknown flag bits");
  MPG_ARG(opts->min_valid_frac >= 0.0 && opts->min_valid_frac <= 1.0, "mpg_regrid_masked_transpose: min_valid_frac must lie in [0, 1]");   // (false for NaN)
  MPG_ARG(!(opts->flags & MPG_MISSING_VALUE) || opts->missing_value == opts->missing_value, "mpg_regrid_masked_transpose: MPG_MISSING_VALUE with a NaN missing_value (use MPG_MISSING_NAN)");
  const int64_t nplanes = (int64_t)nlev * nfields;
  const int gsz = (g_type & MPG_TYPE_F32) ? 4 : 8;
  int64_t ld;   // the gradient's level stride, checked as a destination stride is
  int rc = dst_stride("mpg_regrid_masked_transpose: gradient", h->n_dst, nplanes, gsz, g_level_stride, &ld);
  if (rc) return rc;
  MPG_ARG(h->n_dst == 0 || nplanes <= (INT64_MAX / 8) / h->n_dst, "mpg_regrid_masked_transpose: the workspace cannot be addressed");
  MPG_ARG(h->n_src == 0 || nplanes <= (INT64_MAX / 8) / h->n_src, "mpg_regrid_masked_transpose: the source cannot be addressed");
  // the workspace is written while g and src are read and before dst is: it may overlap none of them
  auto overlaps = [&](const void *p, int64_t bytes) {
    const uintptr_t a = (uintptr_t)work_dev, b = a + (uintptr_t)(nplanes * h->n_dst * 8), c = (uintptr_t)p, d = c + (uintptr_t)bytes;
    return p == (const void *)work_dev || (a < d && c < b);
  };
  MPG_ARG(!overlaps(g_dev, ((nplanes - 1) * ld + h->n_dst) * gsz) && !overlaps(src_dev, nplanes * h->n_src * ((src_type & MPG_TYPE_F32) ? 4 : 8)) &&
              !overlaps(dst_dev, nplanes * h->n_src * ((dst_type & MPG_TYPE_F32) ? 4 : 8)),
          "mpg_regrid_masked_transpose: work_dev must not alias g_dev, src_dev or dst_dev");
  return mpg_k_transpose_masked(h, g_dev, g_type, ld, src_dev, src_type, src_layout, nlev, nfields, dst_dev, dst_type, opts, work_dev,
                                (hipStream_t)hip_stream);
}

int mpg_handle_transpose_stats(mpg_handle h, int64_t *n_referenced, int64_t *max_per_source) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_handle_transpose_stats: NULL handle");
  int rc = mpg_k_transpose_build(h, g_stream);
  if (rc) return rc;
  if (n_referenced) *n_referenced = h->tr_nref;
  if (max_per_source) *max_per_source = h->tr_max;
  return MPG_SUCCESS;
}

int mpg_handle_transpose_build_ms(mpg_handle h, float *ms) {
  MPG_ARG(h && ms, "mpg_handle_transpose_build_ms: NULL argument");
  *ms = h->tr_built ? h->tr_build_ms : 0.f;
  return MPG_SUCCESS;
}

int mpg_regrid_bundle_typed_dev(mpg_handle h, int nfields, const void *const *src_dev, int src_type, int src_layout, int nlev,
                                void *const *dst_dev, int dst_type, double scale, const double *offsets, void *hip_stream) {
  return mpg_regrid_bundle_typed_pitched_dev(h, nfields, src_dev, src_type, src_layout, nlev, dst_dev, dst_type, scale, offsets, 0, hip_stream);
}

int mpg_regrid_bundle_typed_pitched_dev(mpg_handle h, int nfields, const void *const *src_dev, int src_type, int src_layout, int nlev,
                                        void *const *dst_dev, int dst_type, double scale, const double *offsets, int64_t dst_level_stride,
                                        void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h && src_dev && dst_dev, "mpg_regrid_bundle_typed: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid_bundle_typed: nlev and nfields must be >= 1");
  MPG_ARG(src_layout == MPG_LAYOUT_CELL_FAST || src_layout == MPG_LAYOUT_LEV_FAST, "mpg_regrid_bundle_typed: bad src_layout");
  MPG_ARG(src_type >= 0 && src_type <= 3 && dst_type >= 0 && dst_type <= 3, "mpg_regrid_bundle_typed: src_type / dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32, optionally | MPG_TYPE_BE");
  for (int f = 0; f < nfields; ++f) MPG_ARG(dst_dev[f] && (src_dev[f] || h->n_src == 0), "mpg_regrid_bundle_typed: NULL field pointer");
  int64_t ld;   // every field is its own array of nlev planes
  int rc = dst_stride("mpg_regrid_bundle_typed", h->n_dst, nlev, (dst_type & MPG_TYPE_F32) ? 4 : 8, dst_level_stride, &ld);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if (nfields == 1 || h->n_src == 0 || h->n_dst == 0) {   // nothing to share between fields: the plain call, field by field
    for (int f = 0; f < nfields; ++f) {
      rc = mpg_k_apply_typed(h, src_dev[f], src_type, src_layout, nlev, 1, dst_dev[f], dst_type, scale, offsets ? offsets[f] : 0.0, s, FieldTab(), ld);
      if (rc) return rc;
    }
    return MPG_SUCCESS;
  }
  for (int f0 = 0; f0 < nfields; f0 += MPG_TAB_MAX) {   // the pointers travel in the kernels' argument blocks, MPG_TAB_MAX fields per launch
    FieldTab tab;
    tab.n = std::min(MPG_TAB_MAX, nfields - f0);
    for (int k = 0; k < tab.n; ++k) {
      tab.src[k] = src_dev[f0 + k];
      tab.dst[k] = dst_dev[f0 + k];
      tab.off[k] = offsets ? offsets[f0 + k] : 0.0;
    }
    rc = mpg_k_apply_typed(h, nullptr, src_type, src_layout, nlev, tab.n, nullptr, dst_type, scale, 0.0, s, tab, ld);
    if (rc) return rc;
  }
  return MPG_SUCCESS;
}

int mpg_regrid(mpg_handle h, const double *src_host, int src_layout, int nlev, int nfields, double *dst_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && src_host && dst_host, "mpg_regrid: NULL argument");
  MPG_ARG(nlev >= 1 && nfields >= 1, "mpg_regrid: nlev and nfields must be >= 1");
  // float64 in, float64 out through the chunked upload / kernel / download pipeline (mpg_hostpipe.hip): the kernels of
  // mpg_regrid_dev WITH the affine epilogue (scale 1, offset 0), so the same values, and the same bits but for the sign of a zero
  // result: fma(-0.0, 1.0, 0.0) is +0.0, a -0.0 that mpg_regrid_dev stores as it stands comes back as +0.0 here
  return mpg_regrid_typed(h, src_host, 0, src_layout, nlev, nfields, dst_host, 0, 1.0, 0.0);
}

int mpg_rotate_winds_dev(int64_t npts, int nlev, const double *cosa_dev, const double *sina_dev, double *u_dev, double *v_dev,
                         void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(cosa_dev && sina_dev && u_dev && v_dev, "mpg_rotate_winds: NULL argument");
  MPG_ARG(npts >= 0 && nlev >= 1, "mpg_rotate_winds: bad sizes");
  return mpg_k_rotate(npts, nlev, cosa_dev, sina_dev, u_dev, v_dev, (hipStream_t)hip_stream);
}

int mpg_wind_destagger_dev(mpg_handle h1, mpg_handle h2, const double *cosa_dev, const double *sina_dev, const double *umass_dev,
                           const double *vmass_dev, int nlev, void *u_dev, void *v_dev, int dst_type, double *umass_rot_dev, double *vmass_rot_dev,
                           void *hip_stream) {
  return mpg_wind_destagger_pitched_dev(h1, h2, cosa_dev, sina_dev, umass_dev, vmass_dev, nlev, u_dev, v_dev, dst_type, umass_rot_dev, vmass_rot_dev, 0,
                                        hip_stream);
}

int mpg_wind_destagger_pitched_dev(mpg_handle h1, mpg_handle h2, const double *cosa_dev, const double *sina_dev, const double *umass_dev,
                                   const double *vmass_dev, int nlev, void *u_dev, void *v_dev, int dst_type, double *umass_rot_dev,
                                   double *vmass_rot_dev, int64_t dst_level_stride, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h1 || h2, "mpg_wind_destagger: no handle");
  MPG_ARG((cosa_dev == nullptr) == (sina_dev == nullptr), "mpg_wind_destagger: cosa and sina come together");
  const bool rot = cosa_dev != nullptr;
  MPG_ARG(!rot || (h1 && h2), "mpg_wind_destagger: the rotation needs both components (interp.F90:291)");
  MPG_ARG((!h1 || u_dev) && (!h2 || v_dev), "mpg_wind_destagger: NULL destination");
  MPG_ARG((!(h1 || rot) || umass_dev) && (!(h2 || rot) || vmass_dev), "mpg_wind_destagger: NULL mass field");
  MPG_ARG(nlev >= 1, "mpg_wind_destagger: nlev must be >= 1");
  MPG_ARG(dst_type >= 0 && dst_type <= 3, "mpg_wind_destagger: dst_type must be MPG_TYPE_F64 or MPG_TYPE_F32, optionally | MPG_TYPE_BE");
  MPG_ARG((!umass_rot_dev || umass_rot_dev != umass_dev) && (!vmass_rot_dev || vmass_rot_dev != vmass_dev),
          "mpg_wind_destagger: the rotated mass winds cannot replace the inputs (neighbouring tiles read them)");
  MPG_ARG(rot || (!umass_rot_dev && !vmass_rot_dev), "mpg_wind_destagger: rotated mass winds asked for without a rotation");
  int rc;
  if (dst_level_stride != 0) {   // one stride for U [ny][nx+1] and V [ny+1][nx]: at least the plane of each component produced
    const int64_t plane = std::max(h1 ? h1->n_dst : 0, h2 ? h2->n_dst : 0);
    int64_t ld;
    if ((rc = dst_stride("mpg_wind_destagger", plane, nlev, (dst_type & MPG_TYPE_F32) ? 4 : 8, dst_level_stride, &ld))) return rc;
  }
  rc = mpg_k_wind_destagger(h1, h2, cosa_dev, sina_dev, umass_dev, vmass_dev, nlev, u_dev, v_dev, dst_type, umass_rot_dev, vmass_rot_dev,
                            (hipStream_t)hip_stream, dst_level_stride);
  if (rc == MPG_ERR_UNSUPPORTED) mpg_set_error("mpg_wind_destagger: the handles are not the CENTER -> EDGE1 / EDGE2 pair of one grid");
  return rc;
}

// ---- the adjoint of the wind chain: the rotation's, and the fused call (k_wind_transpose.hip) -----------------------------------------------
int mpg_rotate_winds_transpose_dev(int64_t npts, int nlev, const double *cosa_dev, const double *sina_dev, double *gu_dev, double *gv_dev,
                                   void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(cosa_dev && sina_dev && gu_dev && gv_dev, "mpg_rotate_winds_transpose: NULL argument");
  MPG_ARG(npts >= 0 && nlev >= 1, "mpg_rotate_winds_transpose: bad sizes");
  return mpg_k_rotate_transpose(npts, nlev, cosa_dev, sina_dev, gu_dev, gv_dev, (hipStream_t)hip_stream);
}

int mpg_wind_destagger_transpose_dev(mpg_handle h1, mpg_handle h2, const double *cosa_dev, const double *sina_dev, const void *gu_dev,
                                     const void *gv_dev, int src_type, int64_t src_level_stride, int nlev, const double *gumass_rot_dev,
                                     const double *gvmass_rot_dev, double *gumass_dev, double *gvmass_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(h1 || h2, "mpg_wind_destagger_transpose: no handle");
  MPG_ARG((cosa_dev == nullptr) == (sina_dev == nullptr), "mpg_wind_destagger_transpose: cosa and sina come together");
  const bool rot = cosa_dev != nullptr;
  MPG_ARG(!rot || (h1 && h2), "mpg_wind_destagger_transpose: the rotation needs both components (interp.F90:291)");
  MPG_ARG(rot || (!gumass_rot_dev && !gvmass_rot_dev), "mpg_wind_destagger_transpose: a gradient of the rotated mass winds without a rotation");
  MPG_ARG(nlev >= 1, "mpg_wind_destagger_transpose: nlev must be >= 1");
  MPG_ARG(src_type >= 0 && src_type <= 3, "mpg_wind_destagger_transpose: src_type must be MPG_TYPE_F64 or MPG_TYPE_F32");
  if (src_type & MPG_TYPE_BE) {
    mpg_set_error("mpg_wind_destagger_transpose: big-endian values (MPG_TYPE_BE) are not supported");
    return MPG_ERR_UNSUPPORTED;
  }
  MPG_ARG((!h1 || gu_dev) && (!h2 || gv_dev), "mpg_wind_destagger_transpose: NULL gradient of U / V");
  MPG_ARG((!h1 || gumass_dev) && (!h2 || gvmass_dev), "mpg_wind_destagger_transpose: NULL destination");
  for (const void *o : {(const void *)(h1 ? gumass_dev : nullptr), (const void *)(h2 ? gvmass_dev : nullptr)}) {
    if (!o) continue;
    MPG_ARG(o != gu_dev && o != gv_dev && o != (const void *)gumass_rot_dev && o != (const void *)gvmass_rot_dev && o != (const void *)cosa_dev &&
                o != (const void *)sina_dev,
            "mpg_wind_destagger_transpose: a result cannot replace an input (neighbouring points read it)");
  }
  MPG_ARG(!(h1 && h2) || (const void *)gumass_dev != (const void *)gvmass_dev, "mpg_wind_destagger_transpose: the two results are one array");
  // one stride for gU [ny][nx+1] and gV [ny+1][nx]: at least the plane of each component given; 0: each dense
  const int64_t p1 = h1 ? h1->n_dst : 0, p2 = h2 ? h2->n_dst : 0;
  int64_t ldu = p1, ldv = p2;
  if (src_level_stride != 0) {
    int64_t ld;
    int rc = dst_stride("mpg_wind_destagger_transpose: source", std::max(p1, p2), nlev, (src_type & MPG_TYPE_F32) ? 4 : 8, src_level_stride, &ld);
    if (rc) return rc;
    ldu = ldv = ld;
  }
  const int rc = mpg_k_wind_destagger_transpose(h1, h2, cosa_dev, sina_dev, gu_dev, gv_dev, src_type, ldu, ldv, nlev, gumass_rot_dev, gvmass_rot_dev,
                                                gumass_dev, gvmass_dev, (hipStream_t)hip_stream);
  if (rc == MPG_ERR_UNSUPPORTED) mpg_set_error("mpg_wind_destagger: the handles are not the CENTER -> EDGE1 / EDGE2 pair of one grid");
  return rc;
}

int mpg_rotate_winds(int64_t npts, int nlev, const double *cosa_host, const double *sina_host, double *u_host, double *v_host) {
  MPG_CHECK_INIT();
  MPG_ARG(cosa_host && sina_host && u_host && v_host, "mpg_rotate_winds: NULL argument");
  MPG_ARG(npts >= 0 && nlev >= 1, "mpg_rotate_winds: bad sizes");
  TmpBuf<double> cs, uv;
  int rc;
  size_t n = (size_t)npts, nl = n * nlev;
  if ((rc = cs.alloc(2 * n)) || (rc = uv.alloc(2 * nl))) {
    cs.free();
    return rc;
  }
  MPG_HIP(hipMemcpyAsync(cs.p, cosa_host, sizeof(double) * n, hipMemcpyHostToDevice, g_stream));
  MPG_HIP(hipMemcpyAsync(cs.p + n, sina_host, sizeof(double) * n, hipMemcpyHostToDevice, g_stream));
  MPG_HIP(hipMemcpyAsync(uv.p, u_host, sizeof(double) * nl, hipMemcpyHostToDevice, g_stream));
  MPG_HIP(hipMemcpyAsync(uv.p + nl, v_host, sizeof(double) * nl, hipMemcpyHostToDevice, g_stream));
  rc = mpg_k_rotate(npts, nlev, cs.p, cs.p + n, uv.p, uv.p + nl, g_stream);
  if (!rc) {
    MPG_HIP(hipMemcpyAsync(u_host, uv.p, sizeof(double) * nl, hipMemcpyDeviceToHost, g_stream));
    MPG_HIP(hipMemcpyAsync(v_host, uv.p + nl, sizeof(double) * nl, hipMemcpyDeviceToHost, g_stream));
    MPG_HIP(hipStreamSynchronize(g_stream));
  }
  cs.free();
  uv.free();
  return rc;
}

// ---- introspection ----------------------------------------------------------------------------------
// force_csr: a CSR handle even where every mapped row has exactly 3 entries (mpg_reconstruct_store: its consumers take CSR handles only)
static int handle_from_weights(int64_t n_src, int nx_dst, int ny_dst, int64_t nnz, const int32_t *row_host, const int32_t *col_host,
                               const double *S_host, bool force_csr, mpg_handle *out) {
  MPG_CHECK_INIT();
  MPG_ARG(out && (nnz == 0 || (row_host && col_host && S_host)), "mpg_handle_from_weights: NULL argument");
  MPG_ARG(n_src > 0 && n_src < 0x7fffffff && nx_dst > 0 && ny_dst > 0 && nnz >= 0 && nnz < 0x7fffffff,
          "mpg_handle_from_weights: bad sizes");
  int64_t P = (int64_t)nx_dst * ny_dst;
  std::vector<int32_t> rowptr((size_t)P + 1, 0);
  for (int64_t q = 0; q < nnz; ++q) {
    if (row_host[q] < 1 || row_host[q] > P || col_host[q] < 1 || col_host[q] > n_src) {
      mpg_set_error("mpg_handle_from_weights: entry %lld has row %d / col %d outside [1, n_dst] / [1, n_src]", (long long)q,
                    row_host[q], col_host[q]);
      return MPG_ERR_INVALID_ARG;
    }
    rowptr[(size_t)row_host[q]]++;   // count into slot row (1-based) -> exclusive scan below
  }
  int maxlen = 0, minlen_nonempty = 1 << 30;
  for (int64_t p = 0; p < P; ++p) {
    int len = rowptr[(size_t)p + 1];
    if (len > maxlen) maxlen = len;
    if (len > 0 && len < minlen_nonempty) minlen_nonempty = len;
    rowptr[(size_t)p + 1] += rowptr[(size_t)p];
  }
  std::vector<int32_t> col((size_t)nnz + 1);
  std::vector<double> val((size_t)nnz + 1);
  {
    std::vector<int32_t> cur(rowptr.begin(), rowptr.end() - 1);
    for (int64_t q = 0; q < nnz; ++q) {   // stable: keeps the caller's order inside a row
      int32_t r = row_host[q] - 1;
      col[(size_t)cur[r]] = col_host[q] - 1;
      val[(size_t)cur[r]++] = S_host[q];
    }
  }
  mpg_handle_s *h = new mpg_handle_s();
  h->n_src = n_src;
  h->n_dst = P;
  h->nx_dst = nx_dst;
  h->ny_dst = ny_dst;
  h->nnz = nnz;
  h->method = -1;
  int rc = MPG_SUCCESS;
  h->max_row = maxlen;
  if (maxlen == 3 && minlen_nonempty == 3 && !force_csr) {
    // every mapped destination has exactly 3 sources (bilinear on triangles): the fast fixed-3 layout
    h->kind = MPG_KIND_FIXED;
    h->nnz_per_row = 3;
    std::vector<int32_t> idx(3 * (size_t)P, -1);
    std::vector<double> w(3 * (size_t)P, 0.0);
    for (int64_t p = 0; p < P; ++p)
      if (rowptr[(size_t)p + 1] > rowptr[(size_t)p])
        for (int k = 0; k < 3; ++k) {
          idx[(size_t)k * P + p] = col[(size_t)rowptr[(size_t)p] + k];
          w[(size_t)k * P + p] = val[(size_t)rowptr[(size_t)p] + k];
        }
    if (!(rc = h->idx.alloc(3 * (size_t)P)) && !(rc = h->w.alloc(3 * (size_t)P))) {
      MPG_HIP(hipMemcpy(h->idx.p, idx.data(), sizeof(int32_t) * 3 * P, hipMemcpyHostToDevice));
      MPG_HIP(hipMemcpy(h->w.p, w.data(), sizeof(double) * 3 * P, hipMemcpyHostToDevice));
    }
  } else {
    h->kind = MPG_KIND_CSR;
    h->nnz_per_row = 0;
    if (!(rc = h->rowptr.alloc((size_t)P + 1)) && !(rc = h->col.alloc((size_t)nnz + 1)) && !(rc = h->val.alloc((size_t)nnz + 1))) {
      MPG_HIP(hipMemcpy(h->rowptr.p, rowptr.data(), sizeof(int32_t) * (P + 1), hipMemcpyHostToDevice));
      MPG_HIP(hipMemcpy(h->col.p, col.data(), sizeof(int32_t) * (nnz + 1), hipMemcpyHostToDevice));
      MPG_HIP(hipMemcpy(h->val.p, val.data(), sizeof(double) * (nnz + 1), hipMemcpyHostToDevice));
    }
  }
  if (rc) {
    handle_free(h);
    return rc;
  }
  *out = h;
  return MPG_SUCCESS;
}

int mpg_handle_from_weights(int64_t n_src, int nx_dst, int ny_dst, int64_t nnz, const int32_t *row_host, const int32_t *col_host,
                            const double *S_host, mpg_handle *out) {
  return handle_from_weights(n_src, nx_dst, ny_dst, nnz, row_host, col_host, S_host, false, out);
}

int mpg_handle_info(mpg_handle h, int64_t *n_src, int64_t *n_dst, int *nx_dst, int *ny_dst, int *nnz_per_row, int64_t *nnz) {
  MPG_ARG(h, "mpg_handle_info: NULL handle");
  if (n_src) *n_src = h->n_src;
  if (n_dst) *n_dst = h->n_dst;
  if (nx_dst) *nx_dst = h->nx_dst;
  if (ny_dst) *ny_dst = h->ny_dst;
  if (nnz_per_row) *nnz_per_row = h->nnz_per_row;
  if (nnz) *nnz = h->nnz;
  return MPG_SUCCESS;
}

int mpg_handle_store_ms(mpg_handle h, float *ms_total) {
  MPG_ARG(h, "mpg_handle_store_ms: NULL handle");
  if (ms_total) *ms_total = h->store_ms;
  return MPG_SUCCESS;
}

int mpg_handle_store_path(mpg_handle h, int *candidates) {
  MPG_ARG(h, "mpg_handle_store_path: NULL handle");
  if (candidates) *candidates = h->store_path;
  return MPG_SUCCESS;
}

int mpg_handle_store_stats(mpg_handle h, int64_t *stats_host, int n) {
  MPG_ARG(h && stats_host && n >= 1, "mpg_handle_store_stats: bad argument");
  for (int k = 0; k < n; ++k) stats_host[k] = k == 0 ? (int64_t)h->store_path : k < 8 ? h->store_stats[k] : 0;
  return MPG_SUCCESS;
}

int mpg_handle_get_weights(mpg_handle h, int32_t *idx_host, double *w_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && idx_host, "mpg_handle_get_weights: NULL argument");
  MPG_ARG(h->kind == MPG_KIND_FIXED, "mpg_handle_get_weights: handle is CSR, use mpg_handle_get_csr");
  int nz = h->nnz_per_row;
  int64_t P = h->n_dst;
  std::vector<int32_t> ti((size_t)nz * P);
  MPG_HIP(hipMemcpy(ti.data(), h->idx.p, sizeof(int32_t) * nz * P, hipMemcpyDeviceToHost));
  for (int64_t p = 0; p < P; ++p)
    for (int q = 0; q < nz; ++q) idx_host[p * nz + q] = ti[(size_t)q * P + p];
  if (w_host) {
    if (h->w.p) {
      std::vector<double> tw((size_t)nz * P);
      MPG_HIP(hipMemcpy(tw.data(), h->w.p, sizeof(double) * nz * P, hipMemcpyDeviceToHost));
      for (int64_t p = 0; p < P; ++p)
        for (int q = 0; q < nz; ++q) w_host[p * nz + q] = tw[(size_t)q * P + p];
    } else {
      for (int64_t p = 0; p < P * nz; ++p) w_host[p] = idx_host[p] >= 0 ? 1.0 : 0.0;
    }
  }
  return MPG_SUCCESS;
}

int mpg_handle_get_csr(mpg_handle h, int64_t *rowptr_host, int32_t *col_host, double *val_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && rowptr_host, "mpg_handle_get_csr: NULL argument");
  MPG_ARG(h->kind == MPG_KIND_CSR, "mpg_handle_get_csr: handle is not CSR");
  std::vector<int32_t> rp((size_t)h->n_dst + 1);
  MPG_HIP(hipMemcpy(rp.data(), h->rowptr.p, sizeof(int32_t) * (h->n_dst + 1), hipMemcpyDeviceToHost));
  for (int64_t p = 0; p <= h->n_dst; ++p) rowptr_host[p] = rp[p];
  if (col_host) MPG_HIP(hipMemcpy(col_host, h->col.p, sizeof(int32_t) * h->nnz, hipMemcpyDeviceToHost));
  if (val_host) MPG_HIP(hipMemcpy(val_host, h->val.p, sizeof(double) * h->nnz, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

int mpg_handle_kernel_choice(mpg_handle h, int *cell_fast_kernel, int *lev_fast_kernel, int *max_unique) {
  MPG_ARG(h, "mpg_handle_kernel_choice: NULL handle");
  if (cell_fast_kernel) *cell_fast_kernel = h->cf_choice;
  if (lev_fast_kernel) *lev_fast_kernel = h->lf_choice;
  if (max_unique) *max_unique = h->ut_max;
  return MPG_SUCCESS;
}

int mpg_handle_tile_stats(mpg_handle h, int *tile_nx, int *tile_ny, double *reuse, double *line_fill) {
  MPG_ARG(h, "mpg_handle_tile_stats: NULL handle");
  if (h->ut_rpt == 0 || h->ut_total <= 0) {
    mpg_set_error("mpg_handle_tile_stats: the handle has no tile lists (no staged Regrid has run on it yet)");
    return MPG_ERR_INVALID_ARG;
  }
  if (tile_nx) *tile_nx = (h->ut_rpt & 0xFFFFFF) / 1024;   // bit 24: alignment rule of the lists (k_apply_lfu.hip)
  if (tile_ny) *tile_ny = (h->ut_rpt & 0xFFFFFF) % 1024;
  if (reuse) *reuse = 3.0 * (double)h->n_dst / (double)h->ut_total;
  if (line_fill) *line_fill = h->ut_lines > 0 ? (double)h->ut_total / (16.0 * (double)h->ut_lines) : 0.0;
  return MPG_SUCCESS;
}

int mpg_handle_pole_count(mpg_handle h, int64_t *n_points, int *row_len) {
  MPG_ARG(h, "mpg_handle_pole_count: NULL handle");
  if (n_points) *n_points = h->n_pole;
  if (row_len) *row_len = h->pole_len;
  return MPG_SUCCESS;
}

int mpg_handle_get_pole(mpg_handle h, int32_t *dst_id_host, int32_t *src_row_start_host, double *w_pole_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_handle_get_pole: NULL handle");
  if (h->n_pole == 0) return MPG_SUCCESS;
  if (dst_id_host) MPG_HIP(hipMemcpy(dst_id_host, h->pole_dst.p, sizeof(int32_t) * h->n_pole, hipMemcpyDeviceToHost));
  if (src_row_start_host) MPG_HIP(hipMemcpy(src_row_start_host, h->pole_src0.p, sizeof(int32_t) * h->n_pole, hipMemcpyDeviceToHost));
  if (w_pole_host) MPG_HIP(hipMemcpy(w_pole_host, h->pole_w.p, sizeof(double) * h->n_pole, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

// the tile lists of the LDS-staged level-fast kernel hold source ids: re-indexing a handle drops them
static void lf_invalidate(mpg_handle_s *h) {
  h->free_tile_lists();
  h->lf_choice = 0;
  h->cf_choice = 0;
}

// ---- multi-GPU halo support (kernels in k_halo.hip) ----------------------------------------------------
// The source window of a mesh (mpg_mesh_set_source_window) and the in-place re-indexing verbs below are two answers to the
// same question -- which sources does this rank hold -- and do not compose: a handle of a windowed mesh indexes relative to
// the window, which mpg_handle_rebase / _localize / mpg_halo_build would take for global ids.  They refuse such a handle;
// mpg_handle_unique_sources and mpg_handle_source_range report GLOBAL ids whatever the window is.
}  // extern "C"
int64_t mpg_handle_window_first(const mpg_handle_s *h) {   // > 0 offset of the handle's indices, 0 when its mesh is not windowed
  return mpg_handle_is_windowed(h) ? ((const mpg_mesh_s *)h->key.src)->win_first[h->key.source_mesh_loc()] : 0;
}
bool mpg_handle_is_windowed(const mpg_handle_s *h) {
  if (!h->cached || !h->key.source_is_mesh()) return false;
  return ((const mpg_mesh_s *)h->key.src)->win_count[h->key.source_mesh_loc()] >= 0;
}
extern "C" {
#define MPG_NOT_WINDOWED(h, what)                                                                                                  \
  MPG_ARG(!mpg_handle_is_windowed(h), what ": the handle's mesh has a source window (mpg_mesh_set_source_window); a windowed mesh and " \
                                           "in-place re-indexing are alternatives -- reset the window to the whole mesh first")

int mpg_handle_unique_sources(mpg_handle h, int64_t *n_unique, int32_t *ids_host) {
  MPG_CHECK_INIT();
  MPG_ARG(h && n_unique, "mpg_handle_unique_sources: NULL argument");
  MPG_ARG(!h->localized, "mpg_handle_unique_sources: handle already localized");
  MPG_ARG(h->n_pole == 0, "mpg_handle_unique_sources: handles with pole terms (periodic Grid -> Grid) cannot be re-indexed");
  std::vector<int32_t> ids;
  int rc = mpg_k_unique_sources(h, ids, false, g_stream);
  if (rc) return rc;
  const int32_t w0 = (int32_t)mpg_handle_window_first(h);   // window-relative -> global
  if (w0)
    for (int32_t &c : ids) c += w0;
  *n_unique = (int64_t)ids.size();
  if (ids_host && !ids.empty()) memcpy(ids_host, ids.data(), sizeof(int32_t) * ids.size());
  return MPG_SUCCESS;
}

int mpg_handle_localize(mpg_handle h) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_handle_localize: NULL handle");
  MPG_ARG(!h->localized, "mpg_handle_localize: handle already localized");
  MPG_ARG(h->refcount <= 1, "mpg_handle_localize: the handle is shared (a second mpg_regrid_store returned it from the cache); "
                            "re-indexing it in place would corrupt the other holder's indices -- release the other reference first");
  MPG_ARG(h->n_pole == 0, "mpg_handle_localize: handles with pole terms (periodic Grid -> Grid) cannot be re-indexed");
  MPG_NOT_WINDOWED(h, "mpg_handle_localize");
  // a localized handle no longer matches its cache key: detach it
  cache().detach(h);
  std::vector<int32_t> ids;
  lf_invalidate(h);
  return mpg_k_unique_sources(h, ids, true, g_stream);
}

int mpg_handle_rebase(mpg_handle h, int64_t base, int64_t n_local) {
  MPG_CHECK_INIT();
  MPG_ARG(h, "mpg_handle_rebase: NULL handle");
  MPG_ARG(!h->localized, "mpg_handle_rebase: handle already localized");
  MPG_ARG(h->refcount <= 1, "mpg_handle_rebase: the handle is shared (a second mpg_regrid_store returned it from the cache); "
                            "re-indexing it in place would corrupt the other holder's indices -- release the other reference first");
  MPG_ARG(h->n_pole == 0, "mpg_handle_rebase: handles with pole terms (periodic Grid -> Grid) cannot be re-indexed");
  MPG_ARG(base >= 0 && n_local >= 0 && n_local < 0x7fffffff, "mpg_handle_rebase: bad range");
  MPG_NOT_WINDOWED(h, "mpg_handle_rebase");
  cache().detach(h);
  lf_invalidate(h);
  return mpg_k_rebase(h, base, n_local, g_stream);
}

int mpg_tune(const char *key, int value) {
  MPG_ARG(key, "mpg_tune: NULL key");
  store_worker_drain();   // a Store that was begun under the old setting finishes under it: its cache key says so
  int rc = mpg_k_tune(key, value);
  if (rc) mpg_set_error("mpg_tune: unknown key or value out of range: %s=%d", key, value);
  return rc;
}

int mpg_pack_dev(const double *src_dev, int64_t n_src, int nlev, const int32_t *ids_dev, int64_t n_ids, double *dst_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(src_dev && ids_dev && dst_dev, "mpg_pack_dev: NULL argument");
  return mpg_k_pack(src_dev, n_src, nlev, ids_dev, n_ids, dst_dev, (hipStream_t)hip_stream);
}

// ---- device buffers for hosts without a HIP binding of their own (the Fortran driver keeps its fields in HBM between
// the input file and the output file; ESMF owned that storage behind ESMF_FieldCreate / farrayPtr) ---------------------
int mpg_dev_alloc(int64_t nbytes, void **out_dev) {
  MPG_CHECK_INIT();
  MPG_ARG(out_dev && nbytes >= 0, "mpg_dev_alloc: bad argument");
  *out_dev = nullptr;
  if (nbytes == 0) return MPG_SUCCESS;
  if (hipMalloc(out_dev, (size_t)nbytes) != hipSuccess) {   // the library's own caches may be what fills the device
    (void)hipGetLastError();
    mpg_release_caches();
    MPG_HIP(hipMalloc(out_dev, (size_t)nbytes));
  }
  return MPG_SUCCESS;
}

int mpg_dev_free(void *dev) {
  MPG_CHECK_INIT();
  if (dev) MPG_HIP(hipFree(dev));
  return MPG_SUCCESS;
}

int mpg_dev_upload(void *dst_dev, const void *src_host, int64_t nbytes) {
  MPG_CHECK_INIT();
  MPG_ARG(nbytes >= 0 && (nbytes == 0 || (dst_dev && src_host)), "mpg_dev_upload: bad argument");
  if (nbytes) MPG_HIP(hipMemcpy(dst_dev, src_host, (size_t)nbytes, hipMemcpyHostToDevice));
  return MPG_SUCCESS;
}

int mpg_dev_download(void *dst_host, const void *src_dev, int64_t nbytes) {
  MPG_CHECK_INIT();
  MPG_ARG(nbytes >= 0 && (nbytes == 0 || (dst_host && src_dev)), "mpg_dev_download: bad argument");
  if (nbytes) MPG_HIP(hipMemcpy(dst_host, src_dev, (size_t)nbytes, hipMemcpyDeviceToHost));
  return MPG_SUCCESS;
}

// ---- output epilogues (kernels in k_post.hip) ------------------------------------------------------------
int mpg_bswap_dev(void *buf_dev, int64_t n, int elem_size, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(n >= 0 && (n == 0 || buf_dev), "mpg_bswap_dev: NULL argument");
  return mpg_k_bswap(buf_dev, n, elem_size, (hipStream_t)hip_stream);
}

int mpg_post_cast_dev(const double *src_dev, int64_t n, double scale, double offset, float *dst_dev, int dst_be, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(n >= 0 && (n == 0 || (src_dev && dst_dev)), "mpg_post_cast_dev: NULL argument");
  return mpg_k_post_cast(src_dev, n, scale, offset, dst_dev, dst_be != 0, (hipStream_t)hip_stream);
}

int mpg_post_layer_mean_dev(const double *src_dev, int nlevp1, int64_t n_pts, float *dst_dev, int dst_be, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(nlevp1 >= 2 && n_pts >= 0, "mpg_post_layer_mean_dev: needs at least two levels");
  MPG_ARG(n_pts == 0 || (src_dev && dst_dev), "mpg_post_layer_mean_dev: NULL argument");
  return mpg_k_post_layer_mean(src_dev, nlevp1, n_pts, dst_dev, dst_be != 0, (hipStream_t)hip_stream);
}

int mpg_post_ptop_dev(const double *p_hyd_dev, int nlev, int64_t n_pts, double *ptop_host, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(p_hyd_dev && ptop_host && nlev >= 1 && n_pts >= 1, "mpg_post_ptop_dev: bad argument");
  return mpg_k_post_ptop(p_hyd_dev, nlev, n_pts, ptop_host, (hipStream_t)hip_stream);
}

int mpg_post_ptop_parts_dev(const double *p_hyd_dev, int nlev, int64_t n_pts, double *vmax_host, double *candmin_host, int *has_cand_host,
                            void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(p_hyd_dev && vmax_host && candmin_host && has_cand_host && nlev >= 1 && n_pts >= 1, "mpg_post_ptop_parts_dev: bad argument");
  return mpg_k_post_ptop_parts(p_hyd_dev, nlev, n_pts, vmax_host, candmin_host, has_cand_host, (hipStream_t)hip_stream);
}

// Test hook (include/mpassit_amd.h): the device-wide primitives of k_prims.hip on host arrays
int mpg_debug_scan_i32(const int32_t *in_host, int64_t n, int32_t *out_host, long long *sum_host) {
  MPG_CHECK_INIT();
  MPG_ARG(n >= 0 && (in_host || n == 0), "mpg_debug_scan_i32: bad argument");
  if (sum_host) *sum_host = 0;
  if (n == 0) return MPG_SUCCESS;
  hipStream_t s = g_stream;
  TmpBuf<int32_t> in, out;
  TmpBuf<long long> sum;
  int rc;
  if ((rc = in.alloc((size_t)n, s)) || (rc = out.alloc((size_t)n, s)) || (rc = sum.alloc(1, s))) return rc;
  MPG_HIP(hipMemcpyAsync(in.p, in_host, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  if ((rc = mpg_sum_i32_i64(in.p, n, sum.p, s)) || (rc = mpg_scan_excl_i32(in.p, out.p, n, s))) return rc;
  if (out_host) MPG_HIP(hipMemcpyAsync(out_host, out.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
  if (sum_host) MPG_HIP(hipMemcpyAsync(sum_host, sum.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  MPG_HIP(hipStreamSynchronize(s));
  // in place (in == out) is what the Stores do: the same answer
  if (out_host) {
    if ((rc = mpg_scan_excl_i32(in.p, in.p, n, s))) return rc;
    std::vector<int32_t> again((size_t)n);
    MPG_HIP(hipMemcpyAsync(again.data(), in.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    MPG_HIP(hipStreamSynchronize(s));
    if (memcmp(again.data(), out_host, sizeof(int32_t) * (size_t)n) != 0) {
      mpg_set_error("mpg_debug_scan_i32: the in-place scan differs from the out-of-place one");
      return MPG_ERR_HIP;
    }
  }
  return MPG_SUCCESS;
}

}  // extern "C"
