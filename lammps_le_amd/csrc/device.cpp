// device.cpp — HBM allocation for one engine instance (288 GB per MI355X: everything stays resident).
#include "comm.h"
#include "device.h"
#include "bin_inl.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>

namespace lmp_le {

// process-wide, over all registries (test hook lammps_le_test_live_resources)
static std::atomic<long long> live_blocks{0}, live_bytes{0}, live_handles{0};

const DevMem::Rec *DevMem::find(void **field) const {
  for (size_t k = recs.size(); k-- > 0;) if (recs[k].field == field) return &recs[k];
  return nullptr;
}
void DevMem::adopt(void **field, size_t bytes, const char *name, Kind kind) {
  recs.push_back({field, bytes, name, kind});
  if (kind <= HOST) { live_blocks++; live_bytes += (long long)bytes; }
  else live_handles++;
}
void DevMem::alloc_bytes(void **field, size_t bytes, const char *name, bool zero, unsigned host_flags, Kind kind) {
  release_field(field);
  if (kind == HOST) HIP_CHECK(hipHostMalloc(field, bytes, host_flags));
  else HIP_CHECK(hipMalloc(field, bytes));
  adopt(field, bytes, name, kind);
  if (!zero) return;
  // null-stream memset + wait: the engine's streams are non-blocking, i.e. NOT ordered behind the null stream, and
  // a memset that is still pending when the first kernel writes the buffer would wipe that kernel's output
  HIP_CHECK(hipMemset(*field, 0, bytes));
  HIP_CHECK(hipStreamSynchronize(nullptr));
}
void DevMem::stream(hipStream_t &s, const char *name, unsigned flags, int priority) {
  release(s);
  HIP_CHECK(hipStreamCreateWithPriority(&s, flags, priority));      // (priority 0 = what hipStreamCreateWithFlags gives)
  adopt((void **)&s, 0, name, STREAM);
}
void DevMem::event(hipEvent_t &e, const char *name, unsigned flags) {
  release(e);
  HIP_CHECK(hipEventCreateWithFlags(&e, flags));
  adopt((void **)&e, 0, name, EVENT);
}
void DevMem::release_field(void **field) {
  const Rec *f = find(field);
  if (!f) return;
  const Rec r = *f;
  recs.erase(recs.begin() + (f - recs.data()));
  switch (r.kind) {
    case DEVICE: (void)hipFree(*r.field); break;
    case HOST: (void)hipHostFree(*r.field); break;
    case STREAM: (void)hipStreamDestroy((hipStream_t)*r.field); break;
    case EVENT: (void)hipEventDestroy((hipEvent_t)*r.field); break;
  }
  if (r.kind <= HOST) { live_blocks--; live_bytes -= (long long)r.bytes; }
  else live_handles--;
  *r.field = nullptr;
}
void DevMem::release_all(bool blocks_only) {
  for (size_t k = recs.size(); k-- > 0;)
    if (!blocks_only || recs[k].kind <= HOST) release_field(recs[k].field);
}
size_t DevMem::device_bytes() const {
  size_t b = 0;
  for (const Rec &r : recs) if (r.kind == DEVICE) b += r.bytes;
  return b;
}
void DevMem::trace(const char *when, int rank) const {
  const char *env = getenv("LAMMPS_LE_TRACE_ALLOC");
  if (!env || atoi(env) == 0) return;
  static const char *const kinds[] = {"device", "host", "stream", "event"};
  for (const Rec &r : recs)
    fprintf(stderr, "alloc[%s] rank %d %-24s %-6s %p %zu\n", when, rank, r.name, kinds[r.kind], *r.field, r.bytes);
}
void DevMem::live(long long out[3]) { out[0] = live_blocks; out[1] = live_bytes; out[2] = live_handles; }

void dev_alloc_neigh(DeviceState &d, int maxneigh) {
  // (a bead's count word keeps the entries in 16 bits next to the number of bond entries: engine.h NN_BOND_SHIFT)
  if (maxneigh > NN_COUNT_MASK) throw LammpsError("Neighbor list overflow: more than 65535 neighbors per bead");
  d.maxneigh = maxneigh;
  DEV_ALLOC(d.mem, d.neigh, (size_t)maxneigh * d.npad);
}

void dev_alloc(DeviceState &d, int n, int maxtag, int ntypes, int bpa, int maxspecial, const Box &box,
               double cutneigh) {
  if (!d.stream) d.mem.stream(d.stream, "d.stream", hipStreamNonBlocking);
  d.n = n;
  d.npad = ((n + 63) / 64) * 64 + 64;
  d.maxtag = maxtag;
  d.ntypes = ntypes;
  d.bpa = bpa;
  d.maxspecial = maxspecial;
  d.box = box;
  d.ntotal = maxtag;
  if (!d.dd) d.zlo_ext = box.lo[2];
  d.row_tile = (d.dd || getenv("LAMMPS_LE_NO_ROW_TILES")) ? 0 : ROW_TILE;      // (row_id relies on it being ROW_TILE or 0)
  size_t np = d.npad, nt = (size_t)maxtag + 2;
  DEV_ALLOC(d.mem, d.pos, np); DEV_ALLOC(d.mem, d.pos_tmp, np); DEV_ALLOC(d.mem, d.pos_hold, np); DEV_ALLOC(d.mem, d.posf, np);
  d.xhold = d.pos_hold; d.step_rotated = false;
  for (int k = 0; k < 3; k++) { DEV_ALLOC(d.mem, d.v[k], np); DEV_ALLOC(d.mem, d.v_tmp[k], np); DEV_ALLOC(d.mem, d.f[k], np); }
  DEV_ALLOC(d.mem, d.tag, np); DEV_ALLOC(d.mem, d.tag_tmp, np);
  DEV_ALLOC(d.mem, d.img, 3 * np); DEV_ALLOC(d.mem, d.img_tmp, 3 * np);
  DEV_ALLOC(d.mem, d.map, nt); DEV_ALLOC(d.mem, d.type_t, nt); DEV_ALLOC(d.mem, d.crank, nt);
  DEV_ALLOC(d.mem, d.num_bond, nt); DEV_ALLOC(d.mem, d.bond_type, nt * bpa); DEV_ALLOC(d.mem, d.bond_atom, nt * bpa);
  DEV_ALLOC(d.mem, d.nspecial, nt * 3); DEV_ALLOC(d.mem, d.special, nt * (size_t)maxspecial);
  DEV_ALLOC(d.mem, d.num_bond0, nt); DEV_ALLOC(d.mem, d.bond_type0, nt * bpa); DEV_ALLOC(d.mem, d.bond_atom0, nt * bpa);
  if (d.apa > 0) {
    DEV_ALLOC(d.mem, d.angle_pack, (size_t)ANGLE_PACK_COLS * nt * 4);
    d.angle_pack_dirty = true;
    DEV_ALLOC(d.mem, d.num_angle, nt); DEV_ALLOC(d.mem, d.angle_type, nt * d.apa); DEV_ALLOC(d.mem, d.angle_a1, nt * d.apa); DEV_ALLOC(d.mem, d.angle_a2, nt * d.apa);
    DEV_ALLOC(d.mem, d.angle_a3, nt * d.apa);
    d.ecap = d.apa + 8;
    DEV_ALLOC(d.mem, d.eff_n, np); DEV_ALLOC(d.mem, d.eff_rec, np * (size_t)d.ecap);       // by the bead's physical index, records column-major
  }
  if (maxtag >= (1 << BOND_TYPE_SHIFT)) throw LammpsError("MI355X engine: atom IDs must stay below 2^26");
  d.bond_pack_stride = ((1 + bpa) + 3) & ~3;
  DEV_ALLOC(d.mem, d.bond_pack, nt * (size_t)d.bond_pack_stride);
  for (int k = 0; k < 2; k++) DEV_ALLOC(d.mem, d.bond_pack_p[k], np * (size_t)d.bond_pack_stride);
  // cells of edge >= cutneigh
  d.ncells = 1;
  for (int k = 0; k < 3; k++) {
    double extent = (k == 2 && d.dd) ? (d.slab_hi - d.slab_lo) + 2.0 * d.cutghost : box.prd[k];
    d.ncell[k] = cutneigh > 0.0 ? (int)(extent / (k == 0 ? cutneigh / CELL_XSPLIT : cutneigh)) : 1;
    if (d.ncell[k] < 1) d.ncell[k] = 1;
    // keep cells from getting needlessly tiny for bond-only runs
    d.cellinv[k] = d.ncell[k] / extent;
    d.ncells *= d.ncell[k];
  }
  DEV_ALLOC(d.mem, d.cell_of, np); DEV_ALLOC(d.mem, d.cell_count, (size_t)d.ncells + 2); DEV_ALLOC(d.mem, d.cell_start, (size_t)d.ncells + 2);
  DEV_ALLOC(d.mem, d.scan_tmp, (size_t)d.ncells / 1024 + 2); DEV_ALLOC(d.mem, d.perm, np);
  double vol = box.prd[0] * box.prd[1] * box.prd[2];
  double expect = (double)n / vol * 4.18879020478639 * cutneigh * cutneigh * cutneigh;
  int mn = (int)(expect * 1.5) + 24;
  DEV_ALLOC(d.mem, d.numneigh, np);
  DEV_ALLOC(d.mem, d.bpart, (size_t)std::max(bpa, 1) * np);   // >= 1 row: the step kernel loads before it masks
  DEV_ALLOC(d.mem, d.bshift, np);
  dev_alloc_neigh(d, mn);
  DEV_ALLOC(d.mem, d.pairtab, (size_t)6 * (ntypes + 1) * (ntypes + 1));
  d.nred_blocks = (n + 255) / 256 + 8;
  DEV_ALLOC(d.mem, d.partial, (size_t)d.nred_blocks * 16);
  DEV_ALLOC(d.mem, d.partial_a, (size_t)d.nred_blocks * 8);
  DEV_ALLOC(d.mem, d.lgsum, ((size_t)d.nred_blocks + 1) * 16);
  d.mem.alloc_host(d.partial_h, (size_t)d.nred_blocks * 16, "d.partial_h");
  DEV_ALLOC(d.mem, d.flags, NFLAGS);
  d.mem.alloc_host(d.flags_h, FLAG_SEQ_SLOT + 16, "d.flags_h", hipHostMallocMapped | hipHostMallocCoherent);
  for (int k = 0; k < FLAG_SEQ_SLOT + 16; k++) d.flags_h[k] = 0;
  d.flags_seq = 0;
  note_arrays_allocated(d);      // (freshly allocated arrays are zeroed)
  HIP_CHECK(hipHostGetDevicePointer((void **)&d.flags_h_dev, d.flags_h, 0));
  // LE fix scratch
  DEV_ALLOC(d.mem, d.xt, nt);
  DEV_ALLOC(d.mem, d.xht, nt);
  for (int k = 0; k < 16; k++) DEV_ALLOC(d.mem, d.le_i[k], nt);
  for (int k = 0; k < 2; k++) DEV_ALLOC(d.mem, d.le_d[k], nt);
  DEV_ALLOC(d.mem, d.le_bits, 3 * (nt / 64 + 16));     // three masks: base / accepted pairs, partner below, partner above
  DEV_ALLOC(d.mem, d.le_rng_state, (LE_MAX_FIXES + 1) * 100);      // (+ a scratch copy: chained barrier draws of fix extrusion, kernels_le.hip)
  DEV_ALLOC(d.mem, d.le_draws, 2 * nt);      // (fix extrusion with chained barrier draws: up to four per listing, a listing per two beads)
  DEV_ALLOC(d.mem, d.le_list, 4 * nt);
  DEV_ALLOC(d.mem, d.le_scan, std::max(nt, (size_t)d.ncells + 2) / 1024 + 16);
}

bool dev_alloc_halo_window(DeviceState &d, size_t bytes) {
  d.mem.release(d.halo_win);
  // Uncached (else fine-grained) device memory, as RCCL allocates the buffers its peers write: a neighbour GPU stores into
  // this window while kernels of this GPU are running, which ordinary (coarse-grained) device memory is only coherent
  // for at kernel boundaries of ONE device - this GPU's L2 could keep serving a line of the previous exchange.
  for (unsigned flag : {hipDeviceMallocUncached, hipDeviceMallocFinegrained}) {
    if (hipExtMallocWithFlags((void **)&d.halo_win, bytes, flag) == hipSuccess) {
      d.mem.adopt((void **)&d.halo_win, bytes, "d.halo_win", DevMem::DEVICE);
      return true;
    }
    (void)hipGetLastError();
    d.halo_win = nullptr;
  }
  return false;
}

void dd_fast_halo_free(DeviceState &d);   // kernels_dd.hip
// What survives: configuration (dd, slab bounds, apa, lg_bit, newton_pair, ident_order, flags_seq ..), comm_stream with its
// events and the kernel-timing events; those go with the registry, i.e. with the DeviceState.
void dev_free(DeviceState &d) {
  if (d.rng_stream) (void)hipStreamSynchronize(d.rng_stream);
  if (d.stream) (void)hipStreamSynchronize(d.stream);
  dd_fast_halo_free(d);
  for (int k = 0; k < 2; k++) { d.mem.release(d.rng_done[k]); d.mem.release(d.rng_consumed[k]); }
  d.mem.release(d.rng_stream);
  d.mem.release_all(true);
  d.mem.release(d.stream);
  // words that describe freed memory
  d.rng_out = nullptr; d.gather_recv = nullptr; d.halo_flag = nullptr;
  d.rng_W = 0; d.rng_batch_raw[0] = d.rng_batch_raw[1] = 0;
  d.xhold = nullptr; d.step_rotated = false;
  note_positions_replaced(d);
}

void detach_positions(DeviceState &d) {
  if (!d.xhold_alias || !d.pos || d.xhold != d.pos) return;
  HIP_CHECK(hipMemcpyAsync(d.pos_hold, d.pos, (size_t)d.npad * sizeof(double4), hipMemcpyDeviceToDevice, d.stream));
  std::swap(d.pos, d.pos_hold);      // (xhold keeps naming the buffer of the build, now held by pos_hold)
}
void set_xhold_alias(DeviceState &d, bool on) {
  if (!on && d.pos && d.xhold == d.pos) {
    HIP_CHECK(hipMemcpyAsync(d.pos_hold, d.pos, (size_t)d.npad * sizeof(double4), hipMemcpyDeviceToDevice, d.stream));
    d.xhold = d.pos_hold;
  }
  d.xhold_alias = on;
}

// flags reach the host through a mapped pinned page written by a one-wave kernel (a blit-copy of 64 bytes costs
// ~18 us on this stack, a kernel + sync ~5 us)
// `reset` = bit mask of flags that are zeroed right after they were published (saves one memset launch per flag
// and phase: the consumer of a flag is always the host, which reads the published copy)
// The host does not call hipStreamSynchronize for these hand-overs (its wake-up costs 30-50 us, twice per rebuild):
// the kernel writes a sequence number behind the flags and the host spins on the mapped page.
__global__ void k_publish_flags(int *__restrict__ flags, int *__restrict__ host, unsigned reset, int seq) {
  // ONE wavefront: lane k writes flag k, then - behind the barrier and a system-scope release, which on this
  // hardware waits for every outstanding store of the wave - lane 0 writes the sequence number the host spins on.
  // The host must never see the new number next to old flags: flags and number sit in different 64-byte sectors
  // of the mapped page, and stores of one instruction have no order among themselves, hence the separate store.
  // (Sixteen serial stores from one lane cost 10 us over PCIe; this is one round trip.)
  const int k = threadIdx.x;
  if (k < NFLAGS) {
    int v = flags[k];
    __hip_atomic_store(&host[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((reset >> k) & 1u) flags[k] = 0;
  }
  __syncthreads();
  if (k == 0) __hip_atomic_store(&host[FLAG_SEQ_SLOT], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void stream_sync(DeviceState &d) {
  d.host_waits++;
  if (d.comm_watch) d.comm_watch->wait_stream(d.stream);
  else HIP_CHECK(hipStreamSynchronize(d.stream));
}
void publish_flags(DeviceState &d, unsigned reset) {
  const int seq = ++d.flags_seq;
  hipLaunchKernelGGL(k_publish_flags, dim3(1), dim3(64), 0, d.stream, d.flags, d.flags_h_dev, reset, seq);
}
void sync_flags(DeviceState &d, unsigned reset) {
  publish_flags(d, reset);
  wait_flags(d);
}
// waits for the LAST publish_flags (work enqueued behind it keeps running)
void wait_flags(DeviceState &d) {
  const int seq = d.flags_seq;
  static const bool spin = !getenv("LAMMPS_LE_NO_SPIN");
  if (spin) {
    volatile int *h = d.flags_h;
    auto t0 = std::chrono::steady_clock::now();
    long it = 0;
    while (h[FLAG_SEQ_SLOT] != seq) {
      if ((++it & 0xFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) break;   // long-running
    }                                                                            // work (or a fault): block instead
    if (h[FLAG_SEQ_SLOT] == seq) { std::atomic_thread_fence(std::memory_order_acquire); d.host_waits++; return; }   // pairs with the release store
  }
  stream_sync(d);
}

}  // namespace lmp_le
