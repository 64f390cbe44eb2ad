/* Plain-C consumer of the pitched-destination calls of include/mpassit_amd.h (gcc -std=c99 -pedantic, no C++, no Python).
 * Without a GPU it checks the pure arithmetic of mpg_dst_level_stride and stops at mpg_init; on the GPU it regrids a 2-level
 * constant field from the 4-cell tetrahedral Voronoi mesh onto a 13 x 7 global lat-lon grid (91 points per level: every plane
 * off a 128-byte line) into planes mpg_dst_level_stride apart, and checks every plane against the dense call, the pad
 * untouched, and the pitched planes written to a file as the dense bytes. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mpassit_amd.h"

#define CHECK(call)                                                                   \
  do {                                                                                \
    int rc_ = (call);                                                                 \
    if (rc_ != MPG_SUCCESS) {                                                         \
      fprintf(stderr, "FAIL %s -> %d: %s\n", #call, rc_, mpg_last_error());         \
      return 1;                                                                       \
    }                                                                                 \
  } while (0)

int main(int argc, char **argv) {
  int64_t ld = -1;
  CHECK(mpg_dst_level_stride(1905141, MPG_TYPE_F32 | MPG_TYPE_BE, &ld));   /* 1799 x 1059 mass points: no mpg_init needed */
  if (ld != 1905152) {
    fprintf(stderr, "FAIL: stride %lld\n", (long long)ld);
    return 1;
  }
  CHECK(mpg_dst_level_stride(1905141, MPG_TYPE_F64, &ld));
  if (ld != 1905152 || mpg_dst_level_stride(0, MPG_TYPE_F64, &ld) != MPG_ERR_INVALID_ARG ||
      mpg_dst_level_stride(16, MPG_TYPE_F64, NULL) != MPG_ERR_INVALID_ARG) {
    fprintf(stderr, "FAIL: mpg_dst_level_stride\n");
    return 1;
  }
  printf("pitch_smoke: stride arithmetic ok\n");
  CHECK(mpg_init(0)); /* (no GPU: fails here) */
  const double PI = 3.14159265358979323846;
  const double t[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  double latC[4], lonC[4], latV[4], lonV[4];
  for (int i = 0; i < 4; ++i) {
    double n = sqrt(3.0), x = t[i][0] / n, y = t[i][1] / n, z = t[i][2] / n;
    latC[i] = asin(z);
    lonC[i] = atan2(y, x);
    if (lonC[i] < 0) lonC[i] += 2 * PI;
    latV[i] = asin(-z);
    lonV[i] = atan2(-y, -x);
    if (lonV[i] < 0) lonV[i] += 2 * PI;
  }
  int32_t voc[4][3] = {{2, 3, 4}, {1, 4, 3}, {1, 2, 4}, {1, 3, 2}};
  mpg_mesh mesh;
  CHECK(mpg_mesh_create(4, 4, 3, latC, lonC, latV, lonV, &voc[0][0], &mesh));
  enum { NX = 13, NY = 7, NLEV = 2, P = NX * NY };
  double lon[NY][NX], lat[NY][NX], lonc[NY + 1][NX + 1], latc[NY + 1][NX + 1];
  for (int j = 0; j <= NY; ++j)
    for (int i = 0; i <= NX; ++i) {
      lonc[j][i] = -180.0 + 360.0 / NX * i;
      latc[j][i] = -90.0 + 180.0 / NY * j;
      if (i < NX && j < NY) {
        lon[j][i] = -180.0 + 360.0 / NX * (i + 0.5);
        lat[j][i] = -90.0 + 180.0 / NY * (j + 0.5);
      }
    }
  mpg_grid grid;
  CHECK(mpg_grid_create(NX, NY, 1, &lon[0][0], &lat[0][0], &lonc[0][0], &latc[0][0], NULL, NULL, NULL, NULL, &grid));
  mpg_handle rh;
  CHECK(mpg_regrid_store(mesh, MPG_MESHLOC_ELEMENT, grid, MPG_STAGGERLOC_CENTER, MPG_REGRIDMETHOD_BILINEAR, &rh));
  CHECK(mpg_dst_level_stride(P, MPG_TYPE_F64, &ld));
  if (ld != 96 || mpg_regrid_pitched_dev(rh, NULL, MPG_LAYOUT_CELL_FAST, NLEV, 1, NULL, ld, NULL) != MPG_ERR_INVALID_ARG) {
    fprintf(stderr, "FAIL: stride %lld / NULL arguments accepted\n", (long long)ld);
    return 1;
  }
  const double src[NLEV][4] = {{7.5, 7.5, 7.5, 7.5}, {1.0, 2.0, 3.0, 4.0}};
  double dense[NLEV * P], pitched[NLEV * 96], back[NLEV * P];
  void *d_src, *d_dense, *d_pitched;
  CHECK(mpg_dev_alloc(sizeof src, &d_src));
  CHECK(mpg_dev_alloc(sizeof dense, &d_dense));
  CHECK(mpg_dev_alloc(sizeof pitched, &d_pitched));
  CHECK(mpg_dev_upload(d_src, src, sizeof src));
  memset(pitched, 0xff, sizeof pitched); /* NaN pad */
  CHECK(mpg_dev_upload(d_pitched, pitched, sizeof pitched));
  CHECK(mpg_regrid_dev(rh, (const double *)d_src, MPG_LAYOUT_CELL_FAST, NLEV, 1, (double *)d_dense, NULL));
  if (mpg_regrid_pitched_dev(rh, (const double *)d_src, MPG_LAYOUT_CELL_FAST, NLEV, 1, (double *)d_pitched, P - 1, NULL) != MPG_ERR_INVALID_ARG) {
    fprintf(stderr, "FAIL: a stride below the plane was accepted\n");
    return 1;
  }
  CHECK(mpg_regrid_pitched_dev(rh, (const double *)d_src, MPG_LAYOUT_CELL_FAST, NLEV, 1, (double *)d_pitched, ld, NULL));
  CHECK(mpg_dev_download(dense, d_dense, sizeof dense));
  CHECK(mpg_dev_download(pitched, d_pitched, sizeof pitched));
  for (int k = 0; k < NLEV; ++k) {
    if (memcmp(dense + k * P, pitched + k * ld, P * sizeof(double))) {
      fprintf(stderr, "FAIL: plane %d differs from the dense result\n", k);
      return 1;
    }
    for (int64_t i = P; i < ld; ++i) {
      uint64_t bits;
      memcpy(&bits, pitched + k * ld + i, sizeof bits);
      if (bits != ~(uint64_t)0) {
        fprintf(stderr, "FAIL: pad element %lld of plane %d was written\n", (long long)i, k);
        return 1;
      }
    }
  }
  /* the pitched planes -> one dense range of a file */
  const char *path = argc > 1 ? argv[1] : "pitch_smoke.bin";
  FILE *fp = fopen(path, "wb+");
  if (!fp) {
    fprintf(stderr, "FAIL: cannot create %s\n", path);
    return 1;
  }
  memset(back, 0, sizeof back);
  fwrite(back, 1, sizeof back, fp);
  fflush(fp);
  CHECK(mpg_dev_to_file_planes(path, 0, P * (int64_t)sizeof(double), NLEV, d_pitched, ld * (int64_t)sizeof(double), NULL));
  rewind(fp);
  if (fread(back, 1, sizeof back, fp) != sizeof back || memcmp(back, dense, sizeof dense)) {
    fprintf(stderr, "FAIL: the file does not hold the dense bytes\n");
    return 1;
  }
  fclose(fp);
  remove(path);
  CHECK(mpg_dev_free(d_src));
  CHECK(mpg_dev_free(d_dense));
  CHECK(mpg_dev_free(d_pitched));
  CHECK(mpg_handle_release(rh));
  CHECK(mpg_grid_destroy(grid));
  CHECK(mpg_mesh_destroy(mesh));
  CHECK(mpg_finalize());
  printf("pitch_smoke ok\n");
  return 0;
}
