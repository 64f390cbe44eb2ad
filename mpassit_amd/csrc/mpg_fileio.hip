// mpg_file_to_dev / mpg_dev_to_file: a byte range of a file <-> device memory, with nothing converted on the way.
//
// NetCDF classic variables are contiguous big-endian byte ranges (ncio_var_extent).  The reference reads them into host
// arrays with nf90_get_var (converting and byte-swapping every value on one core, input_data.F90:630) and writes the
// results back through nf90_put_var (write_data.F90:1008-1475).  Here the bytes travel file -> pinned staging -> HBM (and
// back) untouched and are turned around on the GPU (mpg_bswap_dev); the Regrid widens / narrows them in its loads and
// stores.  The host side of such a transfer is page-cache work: pread / pwrite are kernel copies that one core cannot
// do at PCIe speed, so a range is cut into chunks that a few threads move independently, each with two pinned staging
// buffers and its own stream (DMA of one chunk overlaps the page-cache copy of the next).
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <thread>

#include "mpg_internal.h"

namespace {
constexpr int NTHREAD = 8;   // most a direction uses; how many it does use: Lane::nt
constexpr size_t CHUNK = (size_t)32 << 20;

// Staging of one direction: NTHREAD x 2 pinned buffers and NTHREAD streams, created on first use and kept for the
// process.  One transfer per direction at a time (a reader and a writer may run concurrently, e.g. a prefetching reader
// thread beside the thread that writes the previous time level).
struct Lane {
  std::mutex mu;
  bool ready = false;
  size_t bufsize = CHUNK;   // bytes of each pinned staging buffer
  int nt = 4;   // worker threads of this direction (read: 8, the page-cache copy of pread scales; write: 4, pwrite into one tmpfs file does not)
  void *buf[NTHREAD][2] = {};
  hipStream_t stream[NTHREAD] = {};
  hipEvent_t done[NTHREAD][2] = {};
  int init_all() {
    for (int t = 0; t < nt; ++t) {   // only the lanes this direction uses: 2 x 32 MB of pinned memory each
      MPG_HIP(hipStreamCreateWithFlags(&stream[t], hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        MPG_HIP(hipHostMalloc(&buf[t][b], bufsize, hipHostMallocDefault));
        MPG_HIP(hipEventCreateWithFlags(&done[t][b], hipEventDisableTiming));
      }
    }
    return MPG_SUCCESS;
  }
  int init() {   // caller holds mu
    if (ready) return MPG_SUCCESS;
    int rc = init_all();
    if (rc) {
      free_all();   // a partial set (e.g. pinned memory exhausted half way) is given back, the next call starts clean
      return rc;
    }
    ready = true;
    return MPG_SUCCESS;
  }
  void release() {
    std::lock_guard<std::mutex> lock(mu);
    free_all();
  }
  void free_all() {
    for (int t = 0; t < NTHREAD; ++t) {
      if (stream[t]) (void)hipStreamDestroy(stream[t]);
      stream[t] = nullptr;
      for (int b = 0; b < 2; ++b) {
        if (buf[t][b]) (void)hipHostFree(buf[t][b]);
        if (done[t][b]) (void)hipEventDestroy(done[t][b]);
        buf[t][b] = nullptr;
        done[t][b] = nullptr;
      }
    }
    ready = false;
  }
};
Lane g_read, g_write;
struct LaneSetup { LaneSetup() { g_read.nt = 8; const char *e = getenv("MPG_IO_READ_THREADS"); if (e && atoi(e) >= 1 && atoi(e) <= NTHREAD) g_read.nt = atoi(e); } } g_lane_setup;

int xfer_full(int fd, bool writing, char *p, size_t n, off_t off) {
  while (n > 0) {
    ssize_t k = writing ? pwrite(fd, p, n, off) : pread(fd, p, n, off);
    if (k <= 0) return -1;
    p += k;
    off += k;
    n -= (size_t)k;
  }
  return 0;
}

// Device side of a chunk written to the file: bytes [lo, lo + n) of the DENSE range, gathered from planes of `plane` bytes that lie
// `pitch` bytes apart in device memory (pitch == plane: one contiguous copy) -- the partial planes at the chunk's two ends one copy
// each, the whole planes between them one 2-D copy.
hipError_t gather_d2h(char *host, const char *dev, size_t lo, size_t n, size_t plane, size_t pitch, hipStream_t s) {
  if (pitch == plane) return hipMemcpyAsync(host, dev + lo, n, hipMemcpyDeviceToHost, s);
  size_t k = lo / plane, in = lo % plane;
  hipError_t e = hipSuccess;
  if (in) {
    const size_t m = n < plane - in ? n : plane - in;
    if ((e = hipMemcpyAsync(host, dev + k * pitch + in, m, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    host += m;
    n -= m;
    ++k;
  }
  const size_t whole = n / plane;
  if (whole) {
    if ((e = hipMemcpy2DAsync(host, plane, dev + k * pitch, pitch, plane, whole, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    host += whole * plane;
    n -= whole * plane;
    k += whole;
  }
  if (n) e = hipMemcpyAsync(host, dev + k * pitch, n, hipMemcpyDeviceToHost, s);
  return e;
}

// error codes of a worker: 0 ok, 1 file I/O, 2 HIP.  plane / pitch: see gather_d2h (to_dev: always dense)
int transfer(Lane &L, int device, int fd, bool to_dev, int64_t offset, int64_t nbytes, char *dev, size_t plane, size_t pitch) {
  const size_t chunk = CHUNK;
  const int64_t nchunk = (nbytes + (int64_t)chunk - 1) / (int64_t)chunk;
  std::atomic<int64_t> next(0);
  std::atomic<int> err(0);
  auto work = [&](int t) {
    if (hipSetDevice(device) != hipSuccess) {
      err = 2;
      return;
    }
    bool used[2] = {false, false};
    for (int turn = 0;; ++turn) {
      const int64_t c = next.fetch_add(1);
      if (c >= nchunk || err.load()) break;
      const int b = turn & 1;
      const size_t lo = (size_t)c * chunk, n = (size_t)(nbytes - (int64_t)lo < (int64_t)chunk ? nbytes - (int64_t)lo : (int64_t)chunk);
      if (used[b] && hipEventSynchronize(L.done[t][b]) != hipSuccess) { err = 2; break; }  // the buffer's previous DMA
      if (to_dev) {
        if (xfer_full(fd, false, (char *)L.buf[t][b], n, (off_t)(offset + (int64_t)lo))) { err = 1; break; }
        if (hipMemcpyAsync(dev + lo, L.buf[t][b], n, hipMemcpyHostToDevice, L.stream[t]) != hipSuccess ||
            hipEventRecord(L.done[t][b], L.stream[t]) != hipSuccess) { err = 2; break; }
        used[b] = true;
      } else {
        if (gather_d2h((char *)L.buf[t][b], dev, lo, n, plane, pitch, L.stream[t]) != hipSuccess ||
            hipStreamSynchronize(L.stream[t]) != hipSuccess) { err = 2; break; }
        if (xfer_full(fd, true, (char *)L.buf[t][b], n, (off_t)(offset + (int64_t)lo))) { err = 1; break; }
      }
    }
    if (hipStreamSynchronize(L.stream[t]) != hipSuccess) err = 2;
  };
  const int nt = nchunk < L.nt ? (int)nchunk : L.nt;
  std::thread th[NTHREAD];
  for (int t = 1; t < nt; ++t) th[t] = std::thread(work, t);
  work(0);
  for (int t = 1; t < nt; ++t) th[t].join();
  return err.load();
}

int run(bool to_dev, const char *path, int64_t offset, int64_t nbytes, void *dev, hipStream_t s, int64_t plane = 0, int64_t pitch = 0) {
  const char *who = to_dev ? "mpg_file_to_dev" : plane ? "mpg_dev_to_file_planes" : "mpg_dev_to_file";   // (the caller's name in errors)
  if (nbytes == 0) return MPG_SUCCESS;
  Lane &L = to_dev ? g_read : g_write;
  std::lock_guard<std::mutex> lock(L.mu);
  int rc = L.init();
  if (rc) return rc;
  MPG_HIP(hipStreamSynchronize(s));  // to_dev: earlier readers of the buffer are done; to file: its producer is
  const int fd = open(path, to_dev ? O_RDONLY : O_WRONLY);
  if (fd < 0) {
    mpg_set_error("%s: cannot open %s", who, path);
    return MPG_ERR_INVALID_ARG;
  }
  int device = 0;
  (void)hipGetDevice(&device);
  if (plane == 0) plane = pitch = nbytes;
  const int e = transfer(L, device, fd, to_dev, offset, nbytes, (char *)dev, (size_t)plane, (size_t)pitch);
  close(fd);
  if (e == 1) {
    mpg_set_error("%s: short %s on %s (offset %lld, %lld bytes)", who, to_dev ? "read" : "write", path,
                  (long long)offset, (long long)nbytes);
    return MPG_ERR_INVALID_ARG;
  }
  if (e == 2) {
    mpg_set_error("%s: HIP transfer failed", who);
    return MPG_ERR_HIP;
  }
  return MPG_SUCCESS;
}
}  // namespace

// mpg_finalize: the staging buffers and streams belong to the device that was current when they were made
void mpg_fileio_release() {
  g_read.release();
  g_write.release();
}

extern "C" int mpg_file_to_dev(const char *path, int64_t offset, int64_t nbytes, void *dst_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(path && offset >= 0 && nbytes >= 0 && (dst_dev || nbytes == 0), "mpg_file_to_dev: bad argument");
  return run(true, path, offset, nbytes, dst_dev, (hipStream_t)hip_stream);
}

extern "C" int mpg_dev_to_file(const char *path, int64_t offset, int64_t nbytes, const void *src_dev, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(path && offset >= 0 && nbytes >= 0 && (src_dev || nbytes == 0), "mpg_dev_to_file: bad argument");
  return run(false, path, offset, nbytes, (void *)src_dev, (hipStream_t)hip_stream);
}

// Pitched level planes (mpg_regrid_*_pitched_dev results) -> one dense byte range of the file: the chunks are cut over the dense
// range as for mpg_dev_to_file, so a large plane is still written by every writer thread, and each chunk is gathered from the planes.
extern "C" int mpg_dev_to_file_planes(const char *path, int64_t offset, int64_t plane_bytes, int64_t nplanes, const void *src_dev,
                                      int64_t src_pitch_bytes, void *hip_stream) {
  MPG_CHECK_INIT();
  MPG_ARG(path && offset >= 0 && plane_bytes >= 0 && nplanes >= 0 && src_pitch_bytes >= plane_bytes, "mpg_dev_to_file_planes: bad argument");
  MPG_ARG(src_dev || plane_bytes == 0 || nplanes == 0, "mpg_dev_to_file_planes: NULL source");
  if (plane_bytes == 0 || nplanes == 0) return MPG_SUCCESS;
  MPG_ARG(nplanes <= INT64_MAX / src_pitch_bytes && offset <= INT64_MAX - plane_bytes * nplanes, "mpg_dev_to_file_planes: range too large");
  return run(false, path, offset, plane_bytes * nplanes, (void *)src_dev, (hipStream_t)hip_stream, plane_bytes, src_pitch_bytes);
}
