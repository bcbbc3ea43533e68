// kernels_min.hip — the per-bead passes of `minimize` (min_style cg | sd) and the force norms of the thermo keywords
// fmax / fnorm.
//
// Reference semantics restated here:
//   MinLineSearch::alpha_step                      src/min_linesearch.cpp:838-875   (k_min_move)
//   the copies x0 = x of the two line searches     src/min_linesearch.cpp:234, :387 (k_min_store)
//   FixMinimize::reset_coords                      src/fix_minimize.cpp:106-130     (k_min_reset_coords)
//   the dot products and maxima of MinCG::iterate, linemin_backtrack, linemin_quadratic, Min::fnorm_sqr / fnorm_inf /
//   fnorm_max and Thermo::compute_fmax / compute_fnorm                              (k_min_dots)
//   the direction update of MinCG::iterate         src/min_cg.cpp:131-134, :155     (k_min_direction)
//   Neighbor::check_distance                       src/neighbor.cpp:1962-2014       (the FLAG_MOVED rule of k_min_move)
//
// The vectors x0, g and h are keyed by atom ID ([3][stride], stride = maxtag + 2): a rebuild permutes the beads and leaves
// them alone.  Sums are block partials added in a fixed order by one workgroup (k_min_collect): no floating-point atomics,
// the same bits on every repetition.
#include "device.h"

namespace lmp_le {

namespace {
constexpr int MBLOCK = 256;

// sums (cols < NSUM) and maxima (the rest) of NV values per thread -> partial[block][MIN_DOT_COLS]
template <int NV, int NSUM>
__device__ __forceinline__ void min_block_reduce(double (&val)[NV], double *__restrict__ partial, int block) {
  __shared__ double red[MBLOCK / 64][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double s = val[k];
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_down(s, off, 64);
      s = k < NSUM ? s + o : fmax(s, o);
    }
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int k = threadIdx.x;
    double s = red[0][k];
    for (int w = 1; w < MBLOCK / 64; w++) s = k < NSUM ? s + red[w][k] : fmax(s, red[w][k]);
    partial[(size_t)block * MIN_DOT_COLS + k] = s;
  }
}
}  // namespace

__global__ __launch_bounds__(MBLOCK) void k_min_store(int n, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                      size_t stride, double *__restrict__ x0) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  if (p >= n) return;
  const double4 r = pos[p];
  const size_t t = (size_t)tag[p];
  x0[t] = r.x; x0[stride + t] = r.y; x0[2 * stride + t] = r.z;
}

// x = x0, then x += alpha * h when alpha > 0 (alpha_step): alpha = 0 restores x0 bit for bit.  The displacement test against
// the positions of the last list build is k_initial_integrate's.
__global__ __launch_bounds__(MBLOCK) void k_min_move(int n, double4 *__restrict__ pos, const int *__restrict__ tag, size_t stride,
                                                     const double *__restrict__ x0, const double *__restrict__ h, double alpha,
                                                     const double4 *__restrict__ xhold, double triggersq, int *__restrict__ flags) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  if (p >= n) return;
  const size_t t = (size_t)tag[p];
  double4 r = pos[p];
  r.x = x0[t]; r.y = x0[stride + t]; r.z = x0[2 * stride + t];
  if (alpha > 0.0) {
    r.x += alpha * h[t];
    r.y += alpha * h[stride + t];
    r.z += alpha * h[2 * stride + t];
  }
  pos[p] = r;
  const double4 o = xhold[p];
  const double dx = r.x - o.x, dy = r.y - o.y, dz = r.z - o.z;
  const double rsq = dx * dx + dy * dy + dz * dz;
  if (rsq > triggersq) flags[FLAG_MOVED] = 1;
}

// behind a rebuild inside a line search: a bead that Domain::pbc wrapped takes its start coordinate along by whole box
// lengths (Domain::minimum_image of x - x0, orthogonal periodic box: src/domain.cpp minimum_image)
__global__ __launch_bounds__(MBLOCK) void k_min_reset_coords(int n, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                             size_t stride, double *__restrict__ x0, Box box) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  if (p >= n) return;
  const size_t t = (size_t)tag[p];
  const double4 r = pos[p];
  const double xc[3] = {r.x, r.y, r.z};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double d0 = xc[c] - x0[c * stride + t];
    double dd = d0;
    if (fabs(dd) > box.half[c]) { if (dd < 0.0) dd += box.prd[c]; else dd -= box.prd[c]; }
    if (dd != d0) x0[c * stride + t] = xc[c] - dd;
  }
}

// one pass over the beads: f.f, f.h, f.g | max |f_i|^2, max |f_ic|, max |h_ic| (MinDotCol)
template <bool HAVE_G, bool HAVE_H>
__global__ __launch_bounds__(MBLOCK) void k_min_dots(int n, const int *__restrict__ tag, size_t stride, const double *__restrict__ fx,
                                                     const double *__restrict__ fy, const double *__restrict__ fz,
                                                     const double *__restrict__ g, const double *__restrict__ h,
                                                     double *__restrict__ partial) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  double val[MIN_DOT_USED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p < n) {
    const double a = fx[p], b = fy[p], c = fz[p];
    const double ff = a * a + b * b + c * c;
    val[MIN_FF] = ff;
    val[MIN_FMAX2] = ff;
    val[MIN_FMAXC] = fmax(fmax(fabs(a), fabs(b)), fabs(c));
    if (HAVE_G || HAVE_H) {
      const size_t t = (size_t)tag[p];
      if (HAVE_H) {
        const double h0 = h[t], h1 = h[stride + t], h2 = h[2 * stride + t];
        val[MIN_FH] = a * h0 + b * h1 + c * h2;
        val[MIN_HMAXC] = fmax(fmax(fabs(h0), fabs(h1)), fabs(h2));
      }
      if (HAVE_G) val[MIN_FG] = a * g[t] + b * g[stride + t] + c * g[2 * stride + t];
    }
  }
  min_block_reduce<MIN_DOT_USED, MIN_NSUM>(val, partial, blockIdx.x);
}

// g = f; h = g + beta * h (MinCG::iterate), or h = f alone (MinSD::iterate, and the start of both); g.h lands in the f.h
// column and max |h_ic| in its own, so the line search that follows needs no pass of its own: there f = g
template <bool CG>
__global__ __launch_bounds__(MBLOCK) void k_min_direction(int n, const int *__restrict__ tag, size_t stride, const double *__restrict__ fx,
                                                          const double *__restrict__ fy, const double *__restrict__ fz,
                                                          double *__restrict__ g, double *__restrict__ h, double beta,
                                                          double *__restrict__ partial) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  double val[MIN_DOT_USED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p < n) {
    const size_t t = (size_t)tag[p];
    const double fc[3] = {fx[p], fy[p], fz[p]};
    double gh = 0.0, hm = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double hc = fc[c];
      if (CG) {
        g[c * stride + t] = fc[c];
        hc = fc[c] + beta * h[c * stride + t];
      }
      h[c * stride + t] = hc;
      gh += fc[c] * hc;
      hm = fmax(hm, fabs(hc));
    }
    val[MIN_FH] = gh;
    val[MIN_HMAXC] = hm;
  }
  if (CG) min_block_reduce<MIN_DOT_USED, MIN_NSUM>(val, partial, blockIdx.x);
}

// the fallback of MinCG::iterate (src/min_cg.cpp:168-169): h = g
__global__ __launch_bounds__(MBLOCK) void k_min_h_is_g(int n, const int *__restrict__ tag, size_t stride, const double *__restrict__ g,
                                                       double *__restrict__ h) {
  const int p = blockIdx.x * MBLOCK + threadIdx.x;
  if (p >= n) return;
  const size_t t = (size_t)tag[p];
  for (int c = 0; c < 3; c++) h[c * stride + t] = g[c * stride + t];
}

// Second stage, ONE workgroup: the columns of the block partials in a fixed order (the scheme of k_colsum: thread (grp, c)
// takes rows grp, grp + G, ..; then the G group results in group order), and the totals other reductions left in device memory
// (MinSources), into one record in mapped host memory.  The flags travel behind it with publish_flags.
__global__ __launch_bounds__(MBLOCK) void k_min_collect(int nb, const double *__restrict__ partial, MinSources src, double *__restrict__ rec) {
  constexpr int W = MIN_DOT_COLS, G = MBLOCK / W;
  __shared__ double part[G][W];
  const int c = threadIdx.x % W, grp = threadIdx.x / W;
  const bool sum = c < MIN_NSUM;
  double s = 0.0;
  if (partial && c < MIN_DOT_USED)      // (columns MIN_DOT_USED .. of the partials are never written: the record holds zeros there)
    for (int b = grp; b < nb; b += G) { const double v = partial[(size_t)b * W + c]; s = sum ? s + v : fmax(s, v); }
  part[grp][c] = s;
  __syncthreads();
  if (threadIdx.x < W) {
    double t = part[0][threadIdx.x];
    for (int k = 1; k < G; k++) t = sum ? t + part[k][threadIdx.x] : fmax(t, part[k][threadIdx.x]);
    __hip_atomic_store(&rec[threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  int at = W;
  for (int k = 0; k < src.n; k++) {
    if ((int)threadIdx.x < src.len[k])
      __hip_atomic_store(&rec[at + threadIdx.x], src.ptr[k][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    at += src.len[k];
  }
}

// ------------------------------------------------------------------------------------------------------------------
static inline int min_blocks(const DeviceState &d) { return std::max(1, (d.n + MBLOCK - 1) / MBLOCK); }
static inline int min_partial_blocks(DeviceState &d) {      // ... checked against the rows of block partials there are
  const int nb = min_blocks(d);
  if (!d.min_partial || (size_t)(nb + 1) * MIN_DOT_COLS > d.mem.capacity(d.min_partial)) throw LammpsError("internal: more blocks than rows of the minimiser's block partials");
  return nb;
}
static inline size_t min_stride(const DeviceState &d) { return (size_t)d.maxtag + 2; }

void min_alloc(DeviceState &d, bool vectors) {
  // one row per block of the largest owned count the other partial tables are sized for (dev_alloc: nred_blocks; the owned
  // count of a slab changes with every migration), and a spare one
  const size_t rows = (size_t)d.nred_blocks + 1;
  if (d.mem.capacity(d.min_partial) < rows * MIN_DOT_COLS) DEV_ALLOC(d.mem, d.min_partial, rows * MIN_DOT_COLS);
  if (!d.min_rec) {
    d.mem.alloc_host(d.min_rec, MIN_REC_MAX, "d.min_rec", hipHostMallocMapped | hipHostMallocCoherent);
    for (int k = 0; k < MIN_REC_MAX; k++) d.min_rec[k] = 0.0;
    HIP_CHECK(hipHostGetDevicePointer((void **)&d.min_rec_dev, d.min_rec, 0));
  }
  if (!vectors) return;
  const size_t len = 3 * min_stride(d);
  DEV_ALLOC(d.mem, d.min_x0, len); DEV_ALLOC(d.mem, d.min_g, len); DEV_ALLOC(d.mem, d.min_h, len);
}
void min_free(DeviceState &d, bool all) {
  if (d.stream) (void)hipStreamSynchronize(d.stream);
  d.mem.release(d.min_x0); d.mem.release(d.min_g); d.mem.release(d.min_h);
  if (!all) return;      // (the partials and the record stay with a handle whose thermo output names fmax / fnorm)
  d.mem.release(d.min_partial); d.mem.release(d.min_rec);
  d.min_rec_dev = nullptr;
}

void launch_min_store(DeviceState &d) {
  hipLaunchKernelGGL(k_min_store, dim3(min_blocks(d)), dim3(MBLOCK), 0, d.stream, d.n, d.pos, d.tag, min_stride(d), d.min_x0);
}
void launch_min_move(DeviceState &d, double alpha, double triggersq) {
  note_positions_replaced(d);      // d.pos is written in place: it leaves the buffer that records the last build
  hipLaunchKernelGGL(k_min_move, dim3(min_blocks(d)), dim3(MBLOCK), 0, d.stream, d.n, d.pos, d.tag, min_stride(d), d.min_x0, d.min_h,
                     alpha, d.xhold, triggersq, d.flags);
}
void launch_min_reset_coords(DeviceState &d) {
  hipLaunchKernelGGL(k_min_reset_coords, dim3(min_blocks(d)), dim3(MBLOCK), 0, d.stream, d.n, d.pos, d.tag, min_stride(d), d.min_x0, d.box);
}
void launch_min_dots(DeviceState &d, bool with_g, bool with_h) {
  const int nb = min_partial_blocks(d);
  if ((with_g || with_h) && !(d.min_g && d.min_h)) throw LammpsError("internal: the minimiser's vectors are not allocated");
  with_flags([&](auto G, auto H) {
    hipLaunchKernelGGL((k_min_dots<G, H>), dim3(nb), dim3(MBLOCK), 0, d.stream, d.n, d.tag, min_stride(d), d.f[0], d.f[1], d.f[2],
                       d.min_g, d.min_h, d.min_partial);
  }, with_g, with_h);
}
void launch_min_direction(DeviceState &d, bool cg, double beta) {
  const int nb = min_partial_blocks(d);
  with_flags([&](auto CG) {
    hipLaunchKernelGGL((k_min_direction<CG>), dim3(nb), dim3(MBLOCK), 0, d.stream, d.n, d.tag, min_stride(d), d.f[0], d.f[1], d.f[2],
                       d.min_g, d.min_h, beta, d.min_partial);
  }, cg);
}
void launch_min_h_is_g(DeviceState &d) {
  hipLaunchKernelGGL(k_min_h_is_g, dim3(min_blocks(d)), dim3(MBLOCK), 0, d.stream, d.n, d.tag, min_stride(d), d.min_g, d.min_h);
}
void launch_min_collect(DeviceState &d, bool dots, const MinSources &src) {
  int total = MIN_DOT_COLS;
  for (int k = 0; k < src.n; k++) {
    if (src.len[k] > MBLOCK) throw LammpsError("internal: a source of the minimiser's record is longer than one workgroup");
    total += src.len[k];
  }
  if (total > MIN_REC_MAX) throw LammpsError("internal: the minimiser's record does not hold its sources");
  hipLaunchKernelGGL(k_min_collect, dim3(1), dim3(MBLOCK), 0, d.stream, dots ? min_partial_blocks(d) : 0, dots ? d.min_partial : (const double *)nullptr, src,
                     d.min_rec_dev);
}

}  // namespace lmp_le
