// kernels_capi.hip — ID-addressed access to the device-resident state for the C-ABI (lammps_*_subset, capi.cpp).
//
// The per-atom arrays live in CELL order and move at every reneighbor; map[tag] -> p links a tag to its slot.  A subset
// gather maps each requested ID to its slot and packs the K rows into a small device buffer that goes to the host in one
// copy; a subset scatter brings K rows up in one copy and writes them into the slots.  Nothing here touches more than the
// K requested rows, so the cost is O(K) whatever the size of the system (src/library.cpp:2225-2363 and :2482-2614 are the
// host loops these replace).
//
// Decomposed runs: map[t] is a slot below d.n only on the rank that owns bead t.  Every rank packs the rows it owns and
// marks them in a `found` column; the caller completes the rows with one K-row all-gather.  The tag-indexed tables (type,
// bonds, specials, angles) are replicated on every rank, so their rows are complete on each rank without a collective.
#include <algorithm>
#include <cstring>

#include "device.h"

namespace lmp_le {

constexpr int CAPI_BLOCK = 256;

// ---- gather: out holds K rows of `count` values (double or int, by prop), then K `found` ints ----
__global__ __launch_bounds__(CAPI_BLOCK) void k_subset_gather(int K, int prop, int count, const int *__restrict__ ids,
                                                              const int *__restrict__ map, int n, int npad,
                                                              const double4 *__restrict__ pos, const double *__restrict__ a0,
                                                              const double *__restrict__ a1, const double *__restrict__ a2,
                                                              const int *__restrict__ img, const int *__restrict__ tab,
                                                              double *outd, int *outi,      // (one block: double or int rows)
                                                              int *__restrict__ found) {
  const int i = blockIdx.x * CAPI_BLOCK + threadIdx.x;
  if (i >= K) return;
  const int t = ids[i];
  if (prop == SUBSET_TAGTAB) {              // tag-indexed table of width `count` (row t), the same on every rank
    for (int j = 0; j < count; j++) outi[(size_t)i * count + j] = tab[(size_t)t * count + j];
    found[i] = 1;
    return;
  }
  const int p = map[t];
  const bool own = p >= 0 && p < n;
  found[i] = own ? 1 : 0;
  if (!own) return;
  switch (prop) {
    case SUBSET_X: {
      const double4 r = pos[p];
      outd[3 * (size_t)i] = r.x; outd[3 * (size_t)i + 1] = r.y; outd[3 * (size_t)i + 2] = r.z;
      break;
    }
    case SUBSET_V3:                         // v or f: three column arrays
      outd[3 * (size_t)i] = a0[p]; outd[3 * (size_t)i + 1] = a1[p]; outd[3 * (size_t)i + 2] = a2[p];
      break;
    case SUBSET_IMG3:
      for (int k = 0; k < 3; k++) outi[3 * (size_t)i + k] = img[(size_t)k * npad + p];
      break;
    case SUBSET_IMG1: {                     // lammps_encode_image_flags
      const int ix = img[p], iy = img[npad + p], iz = img[2 * (size_t)npad + p];
      outi[i] = ((ix + 512) & 1023) | (((iy + 512) & 1023) << 10) | (((iz + 512) & 1023) << 20);
      break;
    }
  }
}

// ---- scatter: in holds K rows of `count` values; each rank writes the rows it owns (type: the by-tag table everywhere,
// the .w word of the position where owned).  IDs are unique (the caller keeps the last of repeated IDs, as the reference's
// sequential loop does) ----
__global__ __launch_bounds__(CAPI_BLOCK) void k_subset_scatter(int K, int prop, const int *__restrict__ ids,
                                                               const int *__restrict__ map, int n, int npad,
                                                               double4 *__restrict__ pos, double *__restrict__ a0,
                                                               double *__restrict__ a1, double *__restrict__ a2,
                                                               int *__restrict__ img, int *__restrict__ type_t,
                                                               const double *ind, const int *ini) {   // (one block)
  const int i = blockIdx.x * CAPI_BLOCK + threadIdx.x;
  if (i >= K) return;
  const int t = ids[i];
  const int p = map[t];
  const bool own = p >= 0 && p < n;
  switch (prop) {
    case SUBSET_X:
      if (own) {
        double4 r = pos[p];                 // .w = type stays
        r.x = ind[3 * (size_t)i]; r.y = ind[3 * (size_t)i + 1]; r.z = ind[3 * (size_t)i + 2];
        pos[p] = r;
      }
      break;
    case SUBSET_V3:
      if (own) { a0[p] = ind[3 * (size_t)i]; a1[p] = ind[3 * (size_t)i + 1]; a2[p] = ind[3 * (size_t)i + 2]; }
      break;
    case SUBSET_IMG3:
      if (own) for (int k = 0; k < 3; k++) img[(size_t)k * npad + p] = ini[3 * (size_t)i + k];
      break;
    case SUBSET_IMG1:                       // lammps_decode_image_flags
      if (own) {
        const int im = ini[i];
        img[p] = (im & 1023) - 512; img[npad + p] = ((im >> 10) & 1023) - 512; img[2 * (size_t)npad + p] = (im >> 20) - 512;
      }
      break;
    case SUBSET_TYPE:
      type_t[t] = ini[i];
      if (own) pos[p].w = (double)ini[i];
      break;
  }
}

// device staging buffer: [K ids][K*count values (8-byte aligned)][K found]
static char *capi_staging(DeviceState &d, size_t bytes) {
  if (bytes > d.mem.capacity(d.capi_buf)) DEV_RESERVE(d.mem, d.capi_buf, std::max(bytes, (size_t)1 << 16));
  return d.capi_buf;
}
static size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

static void subset_views(DeviceState &d, int prop, int which, const double *&a0, const double *&a1, const double *&a2) {
  a0 = a1 = a2 = nullptr;
  if (prop == SUBSET_V3) {
    if (which == 0) settle_velocities(d);
    double *const *src = which == 0 ? d.v : d.f;
    a0 = src[0]; a1 = src[1]; a2 = src[2];
  }
}

void subset_gather(DeviceState &d, int prop, int which, const int *tab, int count, int K, const int *ids, void *out_rows,
                   int *found) {
  const bool isint = prop != SUBSET_X && prop != SUBSET_V3;
  const size_t esz = isint ? sizeof(int) : sizeof(double);
  const size_t o_val = align8((size_t)K * sizeof(int)), o_found = align8(o_val + (size_t)K * count * esz);
  char *buf = capi_staging(d, o_found + (size_t)K * sizeof(int));
  HIP_CHECK(hipMemcpyAsync(buf, ids, (size_t)K * sizeof(int), hipMemcpyHostToDevice, d.stream));
  const double *a0, *a1, *a2;
  subset_views(d, prop, which, a0, a1, a2);
  const int nb = (K + CAPI_BLOCK - 1) / CAPI_BLOCK;
  hipLaunchKernelGGL(k_subset_gather, dim3(nb), dim3(CAPI_BLOCK), 0, d.stream, K, prop, count, (const int *)buf, d.map, d.n,
                     d.npad, d.pos, a0, a1, a2, d.img, tab, (double *)(buf + o_val), (int *)(buf + o_val),
                     (int *)(buf + o_found));
  HIP_CHECK(hipGetLastError());
  // one K-row copy down: the packed rows and their found flags are adjacent
  std::vector<char> h(o_found + (size_t)K * sizeof(int) - o_val);
  HIP_CHECK(hipMemcpyAsync(h.data(), buf + o_val, h.size(), hipMemcpyDeviceToHost, d.stream));
  stream_sync(d);
  memcpy(out_rows, h.data(), (size_t)K * count * esz);
  memcpy(found, h.data() + (o_found - o_val), (size_t)K * sizeof(int));
}

void subset_scatter(DeviceState &d, int prop, int which, int count, int K, const int *ids, const void *rows) {
  const bool isint = prop != SUBSET_X && prop != SUBSET_V3;
  const size_t esz = isint ? sizeof(int) : sizeof(double);
  const size_t o_val = align8((size_t)K * sizeof(int)), bytes = o_val + (size_t)K * count * esz;
  char *buf = capi_staging(d, bytes);
  // one K-row copy up: ids and rows in one staging block
  std::vector<char> h(bytes, 0);
  memcpy(h.data(), ids, (size_t)K * sizeof(int));
  memcpy(h.data() + o_val, rows, (size_t)K * count * esz);
  HIP_CHECK(hipMemcpyAsync(buf, h.data(), bytes, hipMemcpyHostToDevice, d.stream));
  const double *a0, *a1, *a2;
  subset_views(d, prop, which, a0, a1, a2);
  const int nb = (K + CAPI_BLOCK - 1) / CAPI_BLOCK;
  hipLaunchKernelGGL(k_subset_scatter, dim3(nb), dim3(CAPI_BLOCK), 0, d.stream, K, prop, (const int *)buf, d.map, d.n, d.npad,
                     d.pos, (double *)a0, (double *)a1, (double *)a2, d.img, d.type_t, (const double *)(buf + o_val),
                     (const int *)(buf + o_val));
  HIP_CHECK(hipGetLastError());
  stream_sync(d);      // (the staging block `h` goes out of scope: the copy must have completed)
}

}  // namespace lmp_le
