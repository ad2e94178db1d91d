// tcmp_retime_runs.h -- per-run torque-feasible retiming (tcmp_minjerk_runs,
// tcmp_retime_runs_traj, tcmp_plan_retime_runs): tcmp_retime.h's stage with one scale per run
// instead of one for the trajectory.  At a waypoint whose seven velocities are 0 (a gate the
// repair closed, or a reversal of every joint) the min-jerk rows are at rest -- the waypoint
// accelerations are 0 anyway -- so the rows either side are dynamically decoupled and each
// stretch between two such waypoints (a run) may be played at its own speed: x_k = 1 / s_k^2
// from the run's own rows, by tcmp_retime.h's definition (include/tcmp.h states it; DESIGN §3
// restates it; tests/retime_runs_ref.py is the oracle).
//
// The rows' intervals come from k_rt_bounds itself (its per-row record, the same two launches
// of the same instantiation as the uniform stage: d = tau - g is exactly 0 on a zero-rate row
// here too).  k_rt_runs reduces them per run, one wavefront per run, persistent over the runs;
// the host decides every run and uploads the (r, x, s, O, o) table; k_rt_runs_apply scales each
// row by its run's entry, warps psg and runs the mode's torque test.  Two host waits, a third
// for the stand-alone form's output copy or the plan form's commit.
//
// A run is reduced by the 64 lanes of one wavefront: right for a planner's runs (tens to
// thousands of rows, and many of them after a repair); a single run of many millions of rows is
// accepted and reduced correctly, at one wavefront's bandwidth.
#pragma once

namespace {

// a run's entry of the table k_rt_runs_apply reads
struct RtRunTab {
  double r, x, s;  // qd' = qd r, qdd' = qdd x
  double O, o;     // psg' = O + (psg - o) s
};

// is interior waypoint w (0 < w < n_wp - 1) at rest: its gate closed, or all seven of gv_at's
// velocities 0.0 (gv_at's arithmetic, operation for operation: IEEE fp64 on host and device)
__host__ __device__ inline bool rr_rest(const double* wp, long long w, const int* gates) {
#pragma clang fp contract(off)
  if (gates && gates[w] == 0) return true;
  for (int k = 0; k < 7; ++k) {
    const double v0 = (wp[7 * w + k] - wp[7 * (w - 1) + k]) / 1.0;
    const double v1 = (wp[7 * (w + 1) + k] - wp[7 * w + k]) / 1.0;
    const double gv = (v0 * v1 >= 1e-10) ? 0.5 * (v0 + v1) : 0.0;
    if (gv != 0.0) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------
// k_rr_offsets: the plan form's runs on the device (tcmp_minjerk_runs' rule), so that the
// waypoints need not travel to the host first.  One block: 1,024 waypoints' flags at a time
// into LDS, compacted in order by thread 0 -- serial in the rest waypoints, as k_repair_update
// is in the segments: a planner's list (under 10^4 waypoints) takes microseconds.
// dro: [n_runs, off[0 .. n_runs]], at most W + 1 entries.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_rr_offsets(const double* __restrict__ wp, long long W,
                                                     long long ni, const int* __restrict__ gates,
                                                     long long* dro) {
  __shared__ int s_flag[1024];
  const int tid = threadIdx.x;
  long long m = 0;  // (thread 0's) rest waypoints so far
  for (long long b0 = 0; b0 < W; b0 += 1024) {
    const long long w = b0 + tid;
    s_flag[tid] = (w > 0 && w < W - 1 && rr_rest(wp, w, gates)) ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
      const int cnt = (int)(W - b0 < 1024 ? W - b0 : 1024);
      for (int t = 0; t < cnt; ++t)
        if (s_flag[t]) dro[2 + m++] = (b0 + t) * ni;
    }
    __syncthreads();
  }
  if (tid == 0) {
    dro[0] = m + 1;
    dro[1] = 0;
    dro[2 + m] = (W - 1) * ni;
  }
}

// ------------------------------------------------------------------------------------------
// k_rt_runs: a segmented min / max / arg reduction of the rows' intervals over contiguous
// runs.  Wavefront w of the grid's G takes runs w, w + G, ...; its lanes stride the run's rows
// in row order and keep the lowest row among equal bounds (strict <); then the DPP reductions
// of tcmp_device.h.  Ties of x_hi: the lowest row (the minimum of the rows attaining it), whose
// record holds its lowest joint.  rows null (base mode): no constraint.  org[k]: the run's time
// origin psg[off[k] - 1] (psg[0] for run 0; 0 without psg).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rt_runs(const RtRow* __restrict__ rows,
                                                 const double* __restrict__ psg,
                                                 const long long* __restrict__ dro, RtPart* part,
                                                 double* org) {
  const long long n_runs = dro[0];
  const long long* const off = dro + 1;
  const int lane = lane_id();
  const long long G = (long long)gridDim.x * 4;
  for (long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); k < n_runs; k += G) {
    const long long b = off[k], e = off[k + 1];
    double ub = INFINITY, lb = 0.0, ff = INFINITY;
    long long row = b + lane;  // (past the end on a lane without rows: its ub stays +inf)
    int jb = 0;
    unsigned long long ns = 0;
    if (rows) {
      for (long long i = b + lane; i < e; i += 64) {
        const RtRow c = rows[i];
        if (c.ub < ub) {
          ub = c.ub;
          row = i;
          jb = c.jb;
        }
        lb = fmax(lb, c.lb);
        ns += (unsigned long long)(c.flags & 1);
        if ((c.flags & 2) && ff == INFINITY) ff = (double)i;  // rows < 2^53
      }
    }
    const double mn = wave_min(ub), mx = wave_max(lb);
    // the lowest row attaining mn (lane 0's row b while every bound is +inf), and its lane
    const double rmin = wave_min(ub == mn ? (double)row : INFINITY);
    const int la = (int)(((long long)rmin - b) & 63);
    const int ja = __shfl(jb, la);
    const unsigned long long nst = wave_sum_u64(ns);
    const double ffm = wave_min(ff);
    if (lane == 0) {
      RtPart w;
      w.x_hi = mn;
      w.x_lo = mx;
      w.bind_row = (long long)rmin;
      w.bind_joint = ja;
      w.n_static = (long long)nst;
      w.first_fail = ffm < INFINITY ? (long long)ffm : LLONG_MAX;
      w.pad = 0;
      part[k] = w;
      org[k] = psg ? psg[b > 0 ? b - 1 : 0] : 0.0;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_rt_runs_apply: k_rt_apply with the row's own run: the run is the last offset at or below
// the row (binary search), its table entry scales the row (one fp64 multiply each, no
// contraction) and warps psg, then the mode's torque test on the scaled row
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE == 3 ? 1 : 2)))
void k_rt_runs_apply(const double* __restrict__ q, const double* __restrict__ qd,
                     const double* __restrict__ qdd, const double* __restrict__ psg, long long n,
                     double mass, const long long* __restrict__ dro,
                     const RtRunTab* __restrict__ tab, double* oqd, double* oqdd, double* opsg,
                     unsigned long long* first_fail) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const RtRunTab t = tab[stage_find(dro + 1, dro[0], i)];  // off[0] = 0, off[n_runs] = n
  double c[7], v[7], a[7];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      c[k] = q[7 * i + k];
      v[k] = qd[7 * i + k] * t.r;
      a[k] = qdd[7 * i + k] * t.x;
    }
    if (psg) {
      const double p = psg[i];
      opsg[i] = (t.s == 1.0 && t.O == t.o) ? p : t.O + (p - t.o) * t.s;
    }
  }
  stage_store_test<MODE>(c, v, a, mass, i, oqd, oqdd, first_fail, (unsigned long long)i);
}

void rr_clear(tcmp_retime_runs_result* r) {
  memset(r, 0, sizeof(*r));
  r->fail_run = -1;
  r->first_fail_before = r->first_fail_after = -1;
}

// The stage on n >= 0 device rows of 7 (psg: n or null).  The runs are in h->rr_off on the
// device ([n_runs, off[0 .. n_runs]], at most max_runs of them: uploaded by the stand-alone
// form, written by k_rr_offsets for the plan form, whose n_runs the host learns with the
// partials).  runs: cap_runs entries or null.  The inputs are only read, so a status other than
// OK leaves the caller's rows as they were.  Two host waits.
int rr_run(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
           const double* psg, long long n, long long max_runs, int mode, double mass,
           double min_scale, double max_scale, double* oqd, double* oqdd, double* opsg,
           tcmp_retime_run* runs, long long cap_runs, tcmp_retime_runs_result* r) {
  const double x_max = rt_x_max(min_scale), x_cap = rt_x_cap(max_scale);
  r->n_rows = n;
  if (max_runs == 0) {  // no rows
    r->x_min = x_max;
    r->time_ratio = 1.0;
    return 0;
  }
  const unsigned nb = grid_for(n, 256);
  int rc = h->rt_part.ensure((size_t)(nb + 1) * sizeof(RtPart) + 8);
  rc = rc ? rc : h->rr_part.ensure((size_t)max_runs * sizeof(RtPart));
  rc = rc ? rc : h->rr_org.ensure((size_t)max_runs);
  rc = rc ? rc : h->rr_tab.ensure((size_t)max_runs * sizeof(RtRunTab));
  if (rc) return rc;
  RtPart* const dpart = reinterpret_cast<RtPart*>(h->rt_part.p);
  unsigned long long* const dff = reinterpret_cast<unsigned long long*>(dpart + nb + 1);
  RtPart* const drun = reinterpret_cast<RtPart*>(h->rr_part.p);
  RtRunTab* const dtab = reinterpret_cast<RtRunTab*>(h->rr_tab.p);
  RtRow* drows = nullptr;
  // the host side: offsets, partials, origins, then the table
  const size_t o_off = 0, o_part = o_off + (size_t)(max_runs + 2) * sizeof(long long),
               o_org = o_part + (size_t)max_runs * sizeof(RtPart),
               o_tab = o_org + (size_t)max_runs * sizeof(double),
               o_end = o_tab + (size_t)max_runs * sizeof(RtRunTab);
  h->rr_host.resize(o_end);
  long long* const hoff = reinterpret_cast<long long*>(h->rr_host.data() + o_off);
  RtPart* const hpart = reinterpret_cast<RtPart*>(h->rr_host.data() + o_part);
  double* const horg = reinterpret_cast<double*>(h->rr_host.data() + o_org);
  RtRunTab* const htab = reinterpret_cast<RtRunTab*>(h->rr_host.data() + o_tab);
  StageSpan t0(h);
  if (mode != TCMP_TORQUE_BASE) {
    rc = h->rt_zero.ensure((size_t)n * 7);
    rc = rc ? rc : h->rt_g.ensure((size_t)n * 6);
    rc = rc ? rc : h->rr_rows.ensure((size_t)n * sizeof(RtRow));
    if (rc) return rc;
    drows = reinterpret_cast<RtRow*>(h->rr_rows.p);
    HIPCHK(hipMemsetAsync(h->rt_zero.p, 0, (size_t)n * 7 * sizeof(double), h->stream));
    hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_bounds, mode), dim3(nb), dim3(256), 0, h->stream, q,
                       h->rt_zero.p, h->rt_zero.p, n, mass, 0, h->rt_g.p, dpart, (RtRow*)nullptr);
    hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_bounds, mode), dim3(nb), dim3(256), 0, h->stream, q, qd,
                       qdd, n, mass, 1, h->rt_g.p, dpart, drows);
  }
  hipLaunchKernelGGL(k_rt_runs, dim3(std::min<unsigned>(grid_for(max_runs, 4), 4096)), dim3(256),
                     0, h->stream, drows, psg, h->rr_off.p, drun, h->rr_org.p);
  HIPCHK(hipGetLastError());
  if (int rc = download(h, hoff, h->rr_off.p, (size_t)(max_runs + 2))) return rc;
  if (int rc = download(h, hpart, drun, (size_t)max_runs)) return rc;
  if (int rc = download(h, horg, h->rr_org.p, (size_t)max_runs)) return rc;
  t0.end();
  if (int rc_s = sync_stream(h)) return rc_s;
  r->ms = t0.ms();
  const long long nr = hoff[0];
  if (nr < 1 || nr > max_runs) return fail(-5, "run offsets out of range");
  r->n_runs = nr;
  if (runs && cap_runs < nr) return fail(-4, "cap_runs below the number of runs");
  // every run's decision (rt_decide, as rt_run's for the trajectory)
  long long ffb = LLONG_MAX, bad_inf = -1, bad_cap = -1;
  for (long long k = 0; k < nr; ++k) {
    const RtPart& p = hpart[k];
    tcmp_retime_run u;
    memset(&u, 0, sizeof(u));
    u.row_begin = hoff[1 + k];
    u.row_end = hoff[2 + k];
    u.x_hi = p.x_hi;
    u.x_lo = p.x_lo;
    u.n_static = p.n_static;
    u.bind_row = p.x_hi < INFINITY ? p.bind_row : -1;
    u.bind_joint = p.x_hi < INFINITY ? p.bind_joint : -1;
    u.first_fail = p.first_fail == LLONG_MAX ? -1 : p.first_fail;
    if (u.first_fail >= 0) ffb = std::min<long long>(ffb, u.first_fail);
    const RtDecision dec =
        rt_decide(p.x_hi, p.x_lo, x_max, x_cap, min_scale == 1.0, max_scale > 0.0);
    u.status = dec.status;
    if (dec.status == TCMP_RETIME_INFEASIBLE) {
      if (bad_inf < 0) bad_inf = k;
    } else if (dec.status == TCMP_RETIME_OVER_CAP) {
      if (bad_cap < 0) bad_cap = k;
    } else {
      u.x = dec.x;
      u.r = std::sqrt(dec.x);
      u.s = 1.0 / u.r;
    }
    htab[k] = RtRunTab{u.r, u.x, u.s, 0.0, 0.0};
    if (runs) runs[k] = u;
  }
  r->first_fail_before = r->first_fail_after = ffb == LLONG_MAX ? -1 : ffb;
  if (bad_inf >= 0 || bad_cap >= 0) {
    r->status = bad_inf >= 0 ? TCMP_RETIME_INFEASIBLE : TCMP_RETIME_OVER_CAP;
    r->fail_run = bad_inf >= 0 ? bad_inf : bad_cap;
    return 0;
  }
  // the warp's origins and the totals, in run order
  {
#pragma clang fp contract(off)
    double sum = 0.0, x_min = INFINITY;
    for (long long k = 0; k < nr; ++k) {
      RtRunTab& t = htab[k];
      t.o = horg[k];
      t.O = k == 0 ? t.o : htab[k - 1].O + (t.o - htab[k - 1].o) * htab[k - 1].s;
      if (runs) runs[k].t_begin = psg ? t.O : 0.0;
      sum += t.s * (double)(hoff[2 + k] - hoff[1 + k]);
      x_min = std::min(x_min, t.x);
      r->n_scaled += t.x != 1.0;
    }
    r->x_min = x_min;
    r->time_ratio = sum / (double)n;
  }
  r->first_fail_after = -1;
  unsigned long long ff = 0;
  StageSpan t1(h);
  HIPCHK(hipMemcpyAsync(dtab, htab, (size_t)nr * sizeof(RtRunTab), hipMemcpyHostToDevice,
                        h->stream));
  HIPCHK(hipMemsetAsync(dff, 0xff, sizeof(ff), h->stream));
  hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_runs_apply, mode), dim3(nb), dim3(256), 0, h->stream, q, qd,
                     qdd, psg, n, mass, h->rr_off.p, dtab, oqd, oqdd, opsg, dff);
  HIPCHK(hipGetLastError());
  t1.end();
  HIPCHK(hipMemcpyAsync(&ff, dff, sizeof(ff), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  r->ms += t1.ms();
  if (ff != kNoRow) {
    r->first_fail_after = (int64_t)ff;
    r->status = TCMP_RETIME_UNVERIFIED;
  }
  return 0;
}

}  // namespace

extern "C" {

int tcmp_minjerk_runs(const double* waypoints, int64_t n_wp, int64_t ni, const int32_t* gates,
                      int64_t* run_off, int64_t cap, int64_t* n_runs) {
  if (!waypoints || !n_runs || (!run_off && cap > 0)) return fail(-1, "bad arguments");
  if (n_wp < 2) return fail(-1, "fewer than two waypoints");
  if (ni < 1) return fail(-1, "Invalid number of intervals chosen (must be greater than 0)");
  if (n_wp > INT_MAX || ni > INT_MAX) return fail(-1, "trajectory too long");
  std::vector<int64_t> off{0};
  for (int64_t w = 1; w < n_wp - 1; ++w)
    if (rr_rest(waypoints, w, gates)) off.push_back(w * ni);
  off.push_back((n_wp - 1) * ni);
  *n_runs = (int64_t)off.size() - 1;
  if (cap < (int64_t)off.size()) return fail(-4, "run_off too small");
  std::copy(off.begin(), off.end(), run_off);
  return 0;
}

int tcmp_retime_runs_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                          const double* psg, int64_t n, const int64_t* run_off, int64_t n_runs,
                          int32_t torque_mode, double payload_mass, const tcmp_retime_cfg* cfg,
                          double* qd_out, double* qdd_out, double* psg_out,
                          tcmp_retime_run* runs, tcmp_retime_runs_result* res) {
  TCMP_ENTER(h);
  if (!res || n < 0 || n > (1ll << 38) || n_runs < 0 || n_runs > n ||
      (n > 0 && (!q || !qd || !qdd || !qd_out || !qdd_out || !run_off)) ||
      (n > 0 && psg && !psg_out))
    return fail(-1, "bad arguments");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  if ((n == 0) != (n_runs == 0)) return fail(-1, "rows without runs, or runs without rows");
  if (n > 0) {
    if (run_off[0] != 0 || run_off[n_runs] != n) return fail(-1, "run_off must span [0, n]");
    for (int64_t k = 0; k < n_runs; ++k)
      if (run_off[k + 1] <= run_off[k]) return fail(-1, "run_off must ascend strictly");
  }
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  rr_clear(res);
  const long long nr = n_runs;  // (read by the upload below: alive until rr_run's first wait)
  if (n > 0) {
    int rc = rt_out(h, n);
    rc = rc ? rc : h->rr_off.ensure((size_t)n_runs + 2);
    rc = rc ? rc : stage_upload_rows(h, q, qd, qdd, psg, n);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->rr_off.p, &nr, sizeof(nr), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->rr_off.p + 1, run_off, (size_t)(n_runs + 1) * sizeof(long long),
                          hipMemcpyHostToDevice, h->stream));
  }
  if (int rc = rr_run(h, h->rt_in[0].p, h->rt_in[1].p, h->rt_in[2].p, psg ? h->rt_in[3].p : nullptr,
                      n, n_runs, torque_mode, payload_mass, mn, mx, h->rt_o[0].p, h->rt_o[1].p,
                      h->rt_o[2].p, runs, n_runs, res))
    return rc;
  if (res->status != TCMP_RETIME_OK || n == 0) return 0;
  if (int rc = stage_download_rows(h, qd_out, qdd_out, psg ? psg_out : nullptr, n)) return rc;
  return sync_stream(h);
}

int tcmp_plan_retime_runs(tcmp_handle* h, const tcmp_retime_cfg* cfg, tcmp_retime_run* runs,
                          int64_t cap_runs, tcmp_retime_runs_result* res) {
  TCMP_ENTER(h);
  if (!res || (runs && cap_runs < 0)) return fail(-1, "bad arguments");
  if (!h->plan_open) return fail(-1, "no open plan");
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  rr_clear(res);
  const long long W = (long long)h->fin_W, K = (long long)h->fin_K;
  if (!stage_applicable(h) || W < 2 || K % (W - 1) != 0) {
    res->status = TCMP_RETIME_NOT_APPLICABLE;
    return 0;
  }
  const long long ni = K / (W - 1);  // K = (W - 1) ni (k_retrace's tail)
  int rc = rt_out(h, K);
  rc = rc ? rc : h->rr_off.ensure((size_t)W + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_rr_offsets, dim3(1), dim3(1024), 0, h->stream, h->wp.p, W, ni,
                     h->pl_gated ? h->pl_gate.p : (const int*)nullptr, h->rr_off.p);
  if (int rc2 = rr_run(h, h->tq.p, h->tqd.p, h->tqdd.p, h->tpsg.p, K, W - 1, h->P.torque_mode,
                       h->P.mass, mn, mx, h->rt_o[0].p, h->rt_o[1].p, h->rt_o[2].p, runs, cap_runs,
                       res))
    return rc2;
  if (res->status != TCMP_RETIME_OK) return 0;
  res->exec_time_after = h->P.exec_time * res->time_ratio;
  StageSpan t(h);
  if (int rc3 = plan_commit_rows(h, t, K, nullptr, h->rt_o[0].p, h->rt_o[1].p, h->rt_o[2].p,
                                 nullptr))
    return rc3;
  res->ms += t.ms();
  h->fin_status = -1;  // retimed: not again before the next finish
  return 0;
}

}  // extern "C"
