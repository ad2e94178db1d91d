// tcmp_retime.h -- torque-feasible retiming of a trajectory (tcmp_retime_traj, tcmp_plan_retime):
// an opt-in stage after the final validation.  One failing row turns a query into nothing
// (rrt_star.py:208-210); for a fixed geometric path the way out is closed-form.  Playing the
// rows s times slower maps (q, v, a) to (q, v / s, a / s^2), and the rne and dyn torque models
// are M a + C(q, v) v + g, so with x = 1 / s^2
//   tau(q, v sqrt(x), a x) = g(q) + x (tau(q, v, a) - g(q)),
// and the torque test of row i, joint j is an interval in x (include/tcmp.h states it; DESIGN §3
// restates it; tests/retime_ref.py is the oracle).  The largest feasible x is a min / max
// reduction over the rows.
//
// k_rt_bounds is launched twice on the same rows, first with all-zero rates (a zeroed buffer, so
// the compiler sees nothing to fold) to store g, then with the real rates: one instantiation,
// one instruction stream, so equal inputs give equal bits and d = tau - g is exactly 0 on a row
// whose rates are zero and in nov mode, whose test ignores them.  One kernel holds one RNE
// (k_traj_tau already needs a whole SIMD's registers for one).
#pragma once

namespace {

// a block's, then the trajectory's, reduction
struct RtPart {
  double x_hi, x_lo;
  long long bind_row;    // lowest row attaining x_hi (any row while x_hi = +inf)
  long long n_static;
  long long first_fail;  // LLONG_MAX: none
  int bind_joint;
  int pad;
};

// a row's own interval (k_rt_bounds' optional record, the input of the per-run reduction in
// tcmp_retime_runs.h): ub / lb over the six joints, the lowest joint attaining ub, and
// flags bit 0: some |g_j| >= L_j - eps, bit 1: the row fails the test as given
struct RtRow {
  double ub, lb;
  int jb;
  int flags;
};

// the six tested joints' torques as the mode's test sees them: the calls torque_test_m makes
// (torque_ok, torque_ok_dyn), stopped before the comparison with the limits
template <int MODE>
__device__ __forceinline__ void rt_torques(double mass, const double cq[7], const double sq[7],
                                           const double v[7], const double a[7], double t[6]) {
  if constexpr (MODE == TCMP_TORQUE_BASE) {
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = 0.0;
  } else if constexpr (MODE == TCMP_TORQUE_DYN) {
    dyn_torques<true>(cq, sq, v, a, mass, t);
  } else {
    double tau[7];
    if constexpr (MODE == TCMP_TORQUE_NOV) {
      const double z[7] = {0, 0, 0, 0, 0, 0, 0};
      rne<false>(cq, sq, z, z, mass > kPayloadMin ? mass : 0.0, tau);
    } else {
      rne<true>(cq, sq, v, a, mass > kPayloadMin ? mass : 0.0, tau);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i] = tau[i];
  }
}

// ------------------------------------------------------------------------------------------
// k_rt_bounds: one row per thread (rows of 7).  pass 0: the row's torques to g (rows of 6).
// pass 1: the row's interval against g, the wave's minimum / maximum (DPP), the block's
// partial.  Ties of x_hi go to the lowest row, then the lowest joint: lanes and waves are
// scanned in row order with a strict <.  rows (null on the uniform path): every row's own
// interval as well, from this same instruction stream.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE >= 2 ? 1 : 2)))
void k_rt_bounds(const double* __restrict__ q, const double* __restrict__ qd,
                 const double* __restrict__ qdd, long long n, double mass, int pass, double* g,
                 RtPart* part, RtRow* rows) {
  __shared__ RtPart wp[4];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool act = i < n;
  const long long ic = act ? i : n - 1;  // (every lane stays active for the wave reductions)
  double x[7], v[7], a[7], cq[7], sq[7], t[6];
  // every load ahead of the arithmetic: the row pointers' scalar registers are free by then
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    x[k] = q[7 * ic + k];
    v[k] = qd[7 * ic + k];
    a[k] = qdd[7 * ic + k];
  }
  __builtin_amdgcn_sched_barrier(0);
  sincos7(x, cq, sq);
  rt_torques<MODE>(mass, cq, sq, v, a, t);
  if (pass == 0) {
    if (act) {
#pragma unroll
      for (int j = 0; j < 6; ++j) g[6 * i + j] = t[j];
    }
    return;
  }
  double ub = INFINITY, lb = 0.0;
  int jb = 0;
  bool stat = false, bad = false;
  if (act) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double gj = g[6 * i + j], tj = t[j], d = tj - gj;
      const double L = kEffort[j], Lg = L - kRtEps;
      double u, l;
      rt_interval(gj, d, L, u, l);
      if (u < ub) {
        ub = u;
        jb = j;
      }
      lb = fmax(lb, l);
      stat |= fabs(gj) >= Lg;
      bad |= fabs(tj) >= L;
    }
    if (rows) {
      RtRow w;
      w.ub = ub;
      w.lb = lb;
      w.jb = jb;
      w.flags = (stat ? 1 : 0) | (bad ? 2 : 0);
      rows[i] = w;
    }
  }
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const double mn = wave_min(ub), mx = wave_max(lb);
  const int la = wave_min_int(ub == mn ? lane : 63) & 63;
  const int ja = __shfl(jb, la);
  const unsigned long long ns = wave_sum_u64(stat ? 1ull : 0ull);
  const double ff = wave_min(bad ? (double)i : INFINITY);  // rows < 2^53
  if (lane == 0) {
    RtPart w;
    w.x_hi = mn;
    w.x_lo = mx;
    w.bind_row = (long long)blockIdx.x * 256 + wave * 64 + la;
    w.bind_joint = ja;
    w.n_static = (long long)ns;
    w.first_fail = ff < INFINITY ? (long long)ff : LLONG_MAX;
    w.pad = 0;
    wp[wave] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    RtPart b = wp[0];
    for (int w = 1; w < 4; ++w) {
      const RtPart c = wp[w];
      if (c.x_hi < b.x_hi) {
        b.x_hi = c.x_hi;
        b.bind_row = c.bind_row;
        b.bind_joint = c.bind_joint;
      }
      b.x_lo = fmax(b.x_lo, c.x_lo);
      b.n_static += c.n_static;
      b.first_fail = c.first_fail < b.first_fail ? c.first_fail : b.first_fail;
    }
    part[blockIdx.x] = b;
  }
}

// ------------------------------------------------------------------------------------------
// k_rt_reduce: the blocks' partials to one, in one block: thread t scans blocks t, t + 256, ...
// in order, then thread 0 the 256 threads' (the lowest row among equal minima)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rt_reduce(const RtPart* __restrict__ part, int nb,
                                                   RtPart* out) {
  __shared__ RtPart sp[256];
  const int tid = threadIdx.x;
  RtPart b{INFINITY, 0.0, LLONG_MAX, 0, LLONG_MAX, 0, 0};
  for (int k = tid; k < nb; k += 256) {
    const RtPart c = part[k];
    if (c.x_hi < b.x_hi || b.bind_row == LLONG_MAX) {
      b.x_hi = c.x_hi;
      b.bind_row = c.bind_row;
      b.bind_joint = c.bind_joint;
    }
    b.x_lo = fmax(b.x_lo, c.x_lo);
    b.n_static += c.n_static;
    b.first_fail = c.first_fail < b.first_fail ? c.first_fail : b.first_fail;
  }
  sp[tid] = b;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 256; ++k) {
      const RtPart c = sp[k];
      if (c.bind_row == LLONG_MAX) continue;  // a thread without a block
      if (c.x_hi < b.x_hi || (c.x_hi == b.x_hi && c.bind_row < b.bind_row)) {
        b.x_hi = c.x_hi;
        b.bind_row = c.bind_row;
        b.bind_joint = c.bind_joint;
      }
      b.x_lo = fmax(b.x_lo, c.x_lo);
      b.n_static += c.n_static;
      b.first_fail = c.first_fail < b.first_fail ? c.first_fail : b.first_fail;
    }
    *out = b;
  }
}

// ------------------------------------------------------------------------------------------
// k_rt_apply: the three multiplies of row i (one fp64 multiply each, no contraction: x = 1
// keeps every bit), then the mode's torque test on the scaled row
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE == 3 ? 1 : 2)))
void k_rt_apply(const double* __restrict__ q, const double* __restrict__ qd,
                const double* __restrict__ qdd, const double* __restrict__ psg, long long n,
                double mass, double r, double x, double s, double* oqd, double* oqdd,
                double* opsg, unsigned long long* first_fail) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double c[7], v[7], a[7];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      c[k] = q[7 * i + k];
      v[k] = qd[7 * i + k] * r;
      a[k] = qdd[7 * i + k] * x;
    }
    if (psg) opsg[i] = psg[i] * s;
  }
  stage_store_test<MODE>(c, v, a, mass, i, oqd, oqdd, first_fail, (unsigned long long)i);
}

int rt_cfg(const tcmp_retime_cfg* cfg, double* min_scale, double* max_scale) {
  *min_scale = cfg && cfg->min_scale != 0.0 ? cfg->min_scale : 1.0;
  *max_scale = cfg ? cfg->max_scale : 0.0;
  if (!(*min_scale > 0.0 && *min_scale <= 1.0)) return fail(-1, "min_scale outside (0, 1]");
  if (!(*max_scale == 0.0 || (*max_scale >= 1.0 && *max_scale < INFINITY)))
    return fail(-1, "max_scale below 1");
  return 0;
}

// the limits of x from the configuration (one division each, by every caller alike)
double rt_x_max(double min_scale) { return 1.0 / (min_scale * min_scale); }
double rt_x_cap(double max_scale) {
  return max_scale > 0.0 ? 1.0 / (max_scale * max_scale) : 0.0;
}

// The stage on n >= 0 device rows of 7 (psg: n or null): bounds, the host's decision, then the
// scaled rows into oqd / oqdd / opsg and their validation.  The inputs are only read, so a
// status other than OK leaves the caller's rows as they were.  Two host waits.
int rt_run(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
           const double* psg, long long n, int mode, double mass, double min_scale,
           double max_scale, double* oqd, double* oqdd, double* opsg, tcmp_retime_result* r) {
  memset(r, 0, sizeof(*r));
  r->n_rows = n;
  RtPart p{INFINITY, 0.0, -1, 0, LLONG_MAX, 0, 0};
  const unsigned nb = grid_for(n, 256);
  if (int rc = h->rt_part.ensure((size_t)(nb + 1) * sizeof(RtPart) + 8)) return rc;
  RtPart* const dpart = reinterpret_cast<RtPart*>(h->rt_part.p);
  unsigned long long* const dff = reinterpret_cast<unsigned long long*>(dpart + nb + 1);
  StageSpan t0(h);
  if (n > 0 && mode != TCMP_TORQUE_BASE) {
    int rc = h->rt_zero.ensure((size_t)n * 7);
    rc = rc ? rc : h->rt_g.ensure((size_t)n * 6);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->rt_zero.p, 0, (size_t)n * 7 * sizeof(double), h->stream));
    hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_bounds, mode), dim3(nb), dim3(256), 0, h->stream, q,
                       h->rt_zero.p, h->rt_zero.p, n, mass, 0, h->rt_g.p, dpart, (RtRow*)nullptr);
    hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_bounds, mode), dim3(nb), dim3(256), 0, h->stream, q, qd,
                       qdd, n, mass, 1, h->rt_g.p, dpart, (RtRow*)nullptr);
    hipLaunchKernelGGL(k_rt_reduce, dim3(1), dim3(256), 0, h->stream, dpart, (int)nb, dpart + nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&p, dpart + nb, sizeof(p), hipMemcpyDeviceToHost, h->stream));
  }
  t0.end();
  if (int rc_s = sync_stream(h)) return rc_s;
  r->ms = t0.ms();
  r->x_hi = p.x_hi;
  r->x_lo = p.x_lo;
  r->n_static = p.n_static;
  r->bind_row = p.x_hi < INFINITY ? p.bind_row : -1;
  r->bind_joint = p.x_hi < INFINITY ? p.bind_joint : -1;
  r->first_fail_before = r->first_fail_after = p.first_fail == LLONG_MAX ? -1 : p.first_fail;
  const RtDecision dec = rt_decide(p.x_hi, p.x_lo, rt_x_max(min_scale), rt_x_cap(max_scale),
                                   min_scale == 1.0, max_scale > 0.0);
  r->status = dec.status;
  if (dec.status != TCMP_RETIME_OK) return 0;
  r->x = dec.x;
  r->r = std::sqrt(dec.x);
  r->s = 1.0 / r->r;
  r->first_fail_after = -1;
  if (n == 0) return 0;
  unsigned long long ff = 0;
  StageSpan t1(h);
  HIPCHK(hipMemsetAsync(dff, 0xff, sizeof(ff), h->stream));
  hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_apply, mode), dim3(nb), dim3(256), 0, h->stream, q, qd, qdd,
                     psg, n, mass, r->r, r->x, r->s, oqd, oqdd, opsg, dff);
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

int rt_out(tcmp_handle* h, long long n) {
  int rc = h->rt_o[0].ensure((size_t)n * 7);
  rc = rc ? rc : h->rt_o[1].ensure((size_t)n * 7);
  return rc ? rc : h->rt_o[2].ensure((size_t)n);
}

}  // namespace

extern "C" {

int tcmp_retime_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                     const double* psg, int64_t n, int32_t torque_mode, double payload_mass,
                     const tcmp_retime_cfg* cfg, double* qd_out, double* qdd_out,
                     double* psg_out, tcmp_retime_result* res) {
  TCMP_ENTER(h);
  if (!res || n < 0 || n > (1ll << 38) || (n > 0 && (!q || !qd || !qdd || !qd_out || !qdd_out)) ||
      (n > 0 && psg && !psg_out))
    return fail(-1, "bad arguments");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  if (n > 0) {
    int rc = rt_out(h, n);
    rc = rc ? rc : stage_upload_rows(h, q, qd, qdd, psg, n);
    if (rc) return rc;
  }
  if (int rc = rt_run(h, h->rt_in[0].p, h->rt_in[1].p, h->rt_in[2].p, psg ? h->rt_in[3].p : nullptr,
                      n, torque_mode, payload_mass, mn, mx, h->rt_o[0].p, h->rt_o[1].p,
                      h->rt_o[2].p, res))
    return rc;
  if (res->status != TCMP_RETIME_OK || n == 0) return 0;
  if (int rc = stage_download_rows(h, qd_out, qdd_out, psg ? psg_out : nullptr, n)) return rc;
  return sync_stream(h);
}

int tcmp_plan_retime(tcmp_handle* h, const tcmp_retime_cfg* cfg, tcmp_retime_result* res) {
  TCMP_ENTER(h);
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  memset(res, 0, sizeof(*res));
  const long long K = (long long)h->fin_K;
  if (!stage_applicable(h)) {
    res->status = TCMP_RETIME_NOT_APPLICABLE;
    res->bind_row = res->bind_joint = -1;
    res->first_fail_before = res->first_fail_after = -1;
    return 0;
  }
  if (int rc = rt_out(h, K)) return rc;
  if (int rc = rt_run(h, h->tq.p, h->tqd.p, h->tqdd.p, h->tpsg.p, K, h->P.torque_mode, h->P.mass,
                      mn, mx, h->rt_o[0].p, h->rt_o[1].p, h->rt_o[2].p, res))
    return rc;
  if (res->status != TCMP_RETIME_OK) return 0;
  res->exec_time_after = res->s * h->P.exec_time;
  StageSpan t(h);
  if (int rc = plan_commit_rows(h, t, K, nullptr, h->rt_o[0].p, h->rt_o[1].p, h->rt_o[2].p, nullptr))
    return rc;
  res->ms += t.ms();
  h->fin_status = -1;  // retimed: not again before the next finish
  return 0;
}

}  // extern "C"
