// tcmp_retime_profile.h -- torque-limited velocity-profile retiming (tcmp_retime_profile_traj,
// tcmp_plan_retime_profile): tcmp_retime.h's identity with the time scale free to vary along the
// path.  With x = sd^2 and u = sdd (path parameter: the original time) row (q, v, a) becomes
// (q, v sqrt(x), a x + v u) and its torque g + u m + x d, affine in (u, x); rows are linked by
// x_{i+1} = x_i + 2 D_i u_i.  A backward pass over the reachable sets and a forward greedy pass
// give the fastest profile (include/tcmp.h states the definition; DESIGN §3 restates it;
// tests/retime_profile_ref.py is the oracle).
//
// Coefficients: k_rt_bounds pass 0 (one RNE per kernel) launched three times on the same rows
// with the rate buffers (0, 0), (0, qd), (qd, qdd): one instantiation, one instruction stream, so
// m = d = 0 exactly on a row at rest and in nov mode.  k_pf_coef forms the differences.
// k_pf_sweep: one wavefront per trajectory, persistent over the trajectories: the uniform floor
// (64 rows per step), the backward pass (one lane per (upper, lower) pair of lines, the fp64 DPP
// reductions of tcmp_device.h) and the forward pass with the time sums.  The chain over the rows
// is latency-bound: the next row's coefficients are loaded, and its lines divided out, ahead of
// the current row's reduction.  k_pf_apply scales each row by its own (x, u) and runs the mode's
// torque test.  The stand-alone call waits for the device once; the plan form twice (the
// verdict, then the commit).
#pragma once

namespace {

constexpr int kPfBadDelta = 64;  // k_pf_sweep's own status: some D_i is not > 0

// the joint's two lines p - S x <= u <= P - S x (line: it has them, m != 0 and no NaN)
__device__ __forceinline__ void pf_line(double g, double m, double d, double L, bool& line,
                                        double& P, double& S, double& p) {
#pragma clang fp contract(off)
  const double Lg = L - kRtEps;
  line = m != 0.0 && g == g && m == m && d == d;
  const double A = fabs(m), sg = m > 0.0 ? g : -g, sd = m > 0.0 ? d : -d;
  P = (Lg - sg) / A;
  p = (-Lg - sg) / A;
  S = sd / A;
}

// ------------------------------------------------------------------------------------------
// k_pf_coef: one row per thread: (g, m, d) of the six joints from the three passes' torques, and
// whether the row fails the test as given (k_rt_bounds' rule on the full torque)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pf_coef(const double* __restrict__ tg,
                                                 const double* __restrict__ tm,
                                                 const double* __restrict__ td, long long n,
                                                 double* coef, int* bad) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool b = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double g = tg[6 * i + j], t = td[6 * i + j];
    coef[18 * i + j] = g;
    coef[18 * i + 6 + j] = tm[6 * i + j] - g;
    coef[18 * i + 12 + j] = t - g;
    b |= fabs(t) >= kEffort[j];
  }
  bad[i] = b ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_pf_sweep: wavefront w of the grid's G takes trajectories w, w + G, ...  Every branch around
// a wave reduction is wave-uniform (row counts, the trajectory's status), and an INFEASIBLE
// trajectory still runs both passes to their ends.
// Backward pass, lane = 8 k + j: k < 6 / j < 6 are the joints' upper / lower lines, 6 the link's;
// lanes 56 .. 61 carry the direct bounds of joints 0 .. 5; the rest idle.
// Forward pass: lanes 0 .. 5 the joints' upper lines, 6 .. 11 their lower lines.
// hib / lob: the sets, written by lane 0 on the way back and read by the wave on the way forth.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pf_sweep(
    const double* __restrict__ coef, const int* __restrict__ bad, const double* __restrict__ psg,
    const long long* __restrict__ off, long long n_traj, double min_scale, double max_scale,
    double x_max, double x_cap, double* hib, double* lob, double* xo, double* uo, double* po,
    tcmp_retime_profile_result* res) {
#pragma clang fp contract(off)
  const int lane = lane_id();
  const int k = lane >> 3, j = lane & 7, kk = k < 6 ? k : 5, jj = j < 6 ? j : 5;
  const int fj = lane < 12 ? lane % 6 : 0;
  const double Lk = kEffort[kk], Lj = kEffort[jj], Lf = kEffort[fj];
  const long long G = (long long)gridDim.x * 4;
  for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_traj; t += G) {
    const long long b = off[t], n = off[t + 1] - b;
    const double* const C = coef + 18 * b;
    const double* const T = psg ? psg + b : nullptr;
    // ---- the uniform floor: tcmp_retime_traj's reduction and decision
    double ub = INFINITY, lb = 0.0, ff = INFINITY;
    for (long long i = lane; i < n; i += 64) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double u, l;
        rt_interval(C[18 * i + a], C[18 * i + 12 + a], kEffort[a], u, l);
        ub = fmin(ub, u);
        lb = fmax(lb, l);
      }
      if (bad[b + i] && ff == INFINITY) ff = (double)i;  // rows < 2^53
    }
    const double x_hi = wave_min(ub), x_lo = wave_max(lb), ffm = wave_min(ff);
    const RtDecision dec =
        rt_decide(x_hi, x_lo, x_max, x_cap, min_scale == 1.0, max_scale > 0.0);
    const int ust = dec.status;
    const double xu = dec.x;
    const bool anch = ust == TCMP_RETIME_OK;
    const double x_floor = anch ? xu : (max_scale > 0.0 ? x_cap : 1e-6);
    // ---- backward: the reachable sets
    long long fail = -1;
    bool bad_delta = false;
    double hn = 0.0, ln = 0.0;  // row i + 1's set
    double gk = 0, mk = 0, dk = 0, gj = 0, mj = 0, dj = 0, dl = 1.0;
    if (n > 0) {
      const double* c = C + 18 * (n - 1);
      gk = c[kk]; mk = c[6 + kk]; dk = c[12 + kk];
      gj = c[jj]; mj = c[6 + jj]; dj = c[12 + jj];
    }
    for (long long i = n - 1; i >= 0; --i) {
      // this row's lines (off the chain), then the row below's loads
      bool line_k, line_j;
      double Pk, Sk, pk, Pj, Sj, pj, du, dlw;
      pf_line(gk, mk, dk, Lk, line_k, Pk, Sk, pk);
      pf_line(gj, mj, dj, Lj, line_j, Pj, Sj, pj);
      rt_interval(gj, dj, Lj, du, dlw);
      if (!(gj == gj && mj == mj && dj == dj)) {
        du = -INFINITY;
        dlw = INFINITY;
      }
      const bool link = i < n - 1;
      const double dd = 2.0 * dl;  // 2 D_i (unused on the last row)
      if (i > 0) {
        const double* c = C + 18 * (i - 1);
        gk = c[kk]; mk = c[6 + kk]; dk = c[12 + kk];
        gj = c[jj]; mj = c[6 + jj]; dj = c[12 + jj];
        dl = T ? T[i] - T[i - 1] : 1.0;
        bad_delta |= !(dl > 0.0);
      }
      const double Sl = 1.0 / dd, Ph = hn / dd, pl = ln / dd;
      const bool up_ok = k < 6 ? line_k : (k == 6 && link);
      const bool lo_ok = j < 6 ? line_j : (j == 6 && link);
      const double Pu = k < 6 ? Pk : Ph, Su = k < 6 ? Sk : Sl;
      const double pw = j < 6 ? pj : pl, sw = j < 6 ? Sj : Sl;
      const double cc = Su - sw, ee = Pu - pw, bb = ee / cc;
      double lu = INFINITY, ll = -INFINITY;
      if (up_ok && lo_ok) {
        if (cc > 0.0) lu = bb;
        else if (cc < 0.0) ll = bb;
        else if (cc == 0.0 && ee < 0.0) lu = -INFINITY;
      }
      if (k == 7 && j < 6 && !line_j) {
        lu = du;
        ll = dlw;
      }
      double hi = fmin(x_max, wave_min(lu)), lo = fmax(x_floor, wave_max(ll));
      if (anch) {
        hi = fmax(hi, x_floor);
        lo = x_floor;
      } else if (!(lo <= hi) && fail < 0) {
        fail = i;
      }
      if (lane == 0) {
        hib[b + i] = hi;
        lob[b + i] = lo;
      }
      hn = hi;
      ln = lo;
    }
    __threadfence();  // lane 0's sets, before the wave reads them back
    // ---- forward: the greedy profile and the time sums
    const double t0 = (T && n > 0) ? T[0] : 0.0;
    const double ru = anch ? sqrt(xu) : 0.0, ru2 = ru + ru;
    double x = n > 0 ? hib[b] : 0.0, r = sqrt(x), tp = t0, tu = t0, x_min = INFINITY;
    long long n_floor = 0, n_cap = 0;
    double gf = 0, mf = 0, df = 0;
    dl = 1.0;
    if (n > 0) {
      gf = C[fj]; mf = C[6 + fj]; df = C[12 + fj];
    }
    if (n > 1) {
      hn = hib[b + 1];
      ln = lob[b + 1];
      dl = T ? T[1] - T[0] : 1.0;
      bad_delta |= !(dl > 0.0);
    }
    for (long long i = 0; i < n; ++i) {
      bool line;
      double P, S, p;
      pf_line(gf, mf, df, Lf, line, P, S, p);
      const double dd = 2.0 * dl, hc = hn, lc = ln;
      if (i + 1 < n) {
        const double* c = C + 18 * (i + 1);
        gf = c[fj]; mf = c[6 + fj]; df = c[12 + fj];
      }
      if (i + 2 < n) {
        hn = hib[b + i + 2];
        ln = lob[b + i + 2];
        dl = T ? T[i + 2] - T[i + 1] : 1.0;
      }
      const double sx = S * x;
      const double U = wave_min(lane < 6 && line ? P - sx : INFINITY);
      const double W = wave_max(lane >= 6 && lane < 12 && line ? p - sx : -INFINITY);
      double un, xn = x;
      if (i + 1 < n) {
        const double tt = fmin(U, (hc - x) / dd);
        xn = fmin(hc, fmax(lc, x + dd * tt));
        un = (xn - x) / dd;
      } else {
        un = fmin(U, fmax(0.0, W));
      }
      if (lane == 0) {
        xo[b + i] = x;
        uo[b + i] = un;
        po[b + i] = tp;
      }
      x_min = fmin(x_min, x);
      n_floor += x == x_floor;
      n_cap += x == x_max;
      if (i + 1 < n) {
        const double rn = sqrt(xn);
        tp = tp + dd / (r + rn);
        if (anch) tu = tu + dd / ru2;
        x = xn;
        r = rn;
      }
    }
    if (lane == 0) {
      tcmp_retime_profile_result w;
      const bool inf = fail >= 0;
      w.status = bad_delta ? kPfBadDelta : inf ? TCMP_RETIME_INFEASIBLE : TCMP_RETIME_OK;
      w.anchored = anch ? 1 : 0;
      w.uniform_status = ust;
      w.pad = 0;
      w.n_rows = n;
      w.fail_row = fail;
      w.first_fail_before = w.first_fail_after = ffm < INFINITY ? (long long)ffm : -1;
      w.n_at_floor = inf ? 0 : n_floor;
      w.n_at_cap = inf ? 0 : n_cap;
      w.x_uniform = anch ? xu : 0.0;
      w.x_floor = x_floor;
      w.x_min = inf ? 0.0 : n > 0 ? x_min : x_max;
      w.time_before = n > 0 ? (T ? T[n - 1] - T[0] : (double)(n - 1)) : 0.0;
      w.time_after = inf ? 0.0 : tp - t0;
      w.time_uniform = (inf || !anch) ? 0.0 : tu - t0;
      w.exec_time_after = 0.0;
      w.ms = 0.0;
      res[t] = w;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_pf_apply: one row per thread.  The row's trajectory is the last offset at or below it
// (binary search; empty trajectories share an offset with their successor); rows of a trajectory
// that is not OK are skipped.  qd' = qd sqrt(x), qdd' = qdd x + qd u, each product rounded before
// the add; x = 1 and u = 0 copies the row (a sum with +0 would lose the sign of a -0).  Then the
// mode's torque test: the trajectory's first failing row.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE == 3 ? 1 : 2)))
void k_pf_apply(const double* __restrict__ q, const double* __restrict__ qd,
                const double* __restrict__ qdd, long long n, double mass,
                const long long* __restrict__ off, long long n_traj,
                const tcmp_retime_profile_result* __restrict__ res, const double* __restrict__ xs,
                const double* __restrict__ us, double* oqd, double* oqdd,
                unsigned long long* first_fail) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long lo = stage_find(off, n_traj, i);  // off[0] = 0, off[n_traj] = n
  if (res[lo].status != TCMP_RETIME_OK) return;
  double c[7], v[7], a[7];
  {
#pragma clang fp contract(off)
    const double x = xs[i], u = us[i], r = sqrt(x);
    const bool keep = x == 1.0 && u == 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      c[k] = q[7 * i + k];
      const double v0 = qd[7 * i + k], a0 = qdd[7 * i + k];
      const double ax = a0 * x, vu = v0 * u;
      v[k] = keep ? v0 : v0 * r;
      a[k] = keep ? a0 : ax + vu;
    }
  }
  stage_store_test<MODE>(c, v, a, mass, i, oqd, oqdd, first_fail + lo,
                         (unsigned long long)(i - off[lo]));
}

void pf_clear(tcmp_retime_profile_result* r) {
  memset(r, 0, sizeof(*r));
  r->fail_row = r->first_fail_before = r->first_fail_after = -1;
}

// The stage on n > 0 device rows of 7 (psg: n or null) in n_traj >= 1 trajectories whose offsets
// are in h->pf_off: the coefficients into h->pf_coef, the profile into h->pf_x / pf_u, the new
// rows into h->rt_o[0..2], the records into h->pf_res and the new rows' first failing rows into
// h->pf_ff.  Everything is enqueued; nothing waits.  The inputs are only read.
int pf_enqueue(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
               const double* psg, long long n, long long n_traj, int mode, double mass,
               double min_scale, double max_scale) {
  int rc = rt_out(h, n);
  for (auto* b : {&h->pf_hi, &h->pf_lo, &h->pf_x, &h->pf_u}) rc = rc ? rc : b->ensure((size_t)n);
  rc = rc ? rc : h->pf_coef.ensure((size_t)n * 18);
  rc = rc ? rc : h->pf_bad.ensure((size_t)n);
  rc = rc ? rc : h->pf_ff.ensure((size_t)n_traj);
  rc = rc ? rc : h->pf_res.ensure((size_t)n_traj * sizeof(tcmp_retime_profile_result));
  if (rc) return rc;
  const unsigned nb = grid_for(n, 256);
  if (mode != TCMP_TORQUE_BASE) {
    rc = h->rt_zero.ensure((size_t)n * 7);
    for (int k = 0; k < 3; ++k) rc = rc ? rc : h->pf_t[k].ensure((size_t)n * 6);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->rt_zero.p, 0, (size_t)n * 7 * sizeof(double), h->stream));
    const double* rates[3][2] = {{h->rt_zero.p, h->rt_zero.p}, {h->rt_zero.p, qd}, {qd, qdd}};
    for (int k = 0; k < 3; ++k)
      hipLaunchKernelGGL(TCMP_BY_MODE(k_rt_bounds, mode), dim3(nb), dim3(256), 0, h->stream, q,
                         rates[k][0], rates[k][1], n, mass, 0, h->pf_t[k].p, (RtPart*)nullptr,
                         (RtRow*)nullptr);
    hipLaunchKernelGGL(k_pf_coef, dim3(nb), dim3(256), 0, h->stream, h->pf_t[0].p, h->pf_t[1].p,
                       h->pf_t[2].p, n, h->pf_coef.p, h->pf_bad.p);
  } else {
    HIPCHK(hipMemsetAsync(h->pf_coef.p, 0, (size_t)n * 18 * sizeof(double), h->stream));
    HIPCHK(hipMemsetAsync(h->pf_bad.p, 0, (size_t)n * sizeof(int), h->stream));
  }
  tcmp_retime_profile_result* const dres =
      reinterpret_cast<tcmp_retime_profile_result*>(h->pf_res.p);
  const double x_max = rt_x_max(min_scale), x_cap = rt_x_cap(max_scale);
  hipLaunchKernelGGL(k_pf_sweep, dim3(std::min<unsigned>(grid_for(n_traj, 4), 4096)), dim3(256), 0,
                     h->stream, h->pf_coef.p, h->pf_bad.p, psg, h->pf_off.p, n_traj, min_scale,
                     max_scale, x_max, x_cap, h->pf_hi.p, h->pf_lo.p, h->pf_x.p, h->pf_u.p,
                     h->rt_o[2].p, dres);
  HIPCHK(hipMemsetAsync(h->pf_ff.p, 0xff, (size_t)n_traj * sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(TCMP_BY_MODE(k_pf_apply, mode), dim3(nb), dim3(256), 0, h->stream, q, qd, qdd,
                     n, mass, h->pf_off.p, n_traj, dres, h->pf_x.p, h->pf_u.p, h->rt_o[0].p,
                     h->rt_o[1].p, h->pf_ff.p);
  HIPCHK(hipGetLastError());
  return 0;
}

// the host's part of a trajectory's record once the device's and its first failing row are here
int pf_verdict(tcmp_retime_profile_result* r, unsigned long long ff) {
  if (r->status == kPfBadDelta) return fail(-1, "psg must ascend strictly inside a trajectory");
  if (r->status == TCMP_RETIME_OK) {
    r->first_fail_after = -1;
    if (ff != kNoRow) {
      r->first_fail_after = (int64_t)ff;
      r->status = TCMP_RETIME_UNVERIFIED;
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int tcmp_retime_profile_traj(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                             const double* psg, const int64_t* traj_off, int64_t n_traj,
                             int32_t torque_mode, double payload_mass, const tcmp_retime_cfg* cfg,
                             double* qd_out, double* qdd_out, double* psg_out, double* x_out,
                             double* u_out, double* coef_out, tcmp_retime_profile_result* results,
                             double* ms) {
  TCMP_ENTER(h);
  if (ms) *ms = 0.0;
  if (n_traj < 0 || n_traj > (1ll << 31) || (n_traj > 0 && (!traj_off || !results)))
    return fail(-1, "bad arguments");
  if (torque_mode < 0 || torque_mode > 3) return fail(-1, "unknown torque mode");
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  if (n_traj == 0) return 0;
  if (traj_off[0] != 0) return fail(-1, "traj_off must start at 0");
  for (int64_t t = 0; t < n_traj; ++t)
    if (traj_off[t + 1] < traj_off[t]) return fail(-1, "traj_off must ascend");
  const long long n = traj_off[n_traj];
  if (n > (1ll << 38) || (n > 0 && (!q || !qd || !qdd || !qd_out || !qdd_out)) ||
      (n > 0 && psg && !psg_out))
    return fail(-1, "bad arguments");
  if (psg)
    for (int64_t t = 0; t < n_traj; ++t)
      for (int64_t i = traj_off[t]; i + 1 < traj_off[t + 1]; ++i)
        if (!(psg[i + 1] - psg[i] > 0.0))
          return fail(-1, "psg must ascend strictly inside a trajectory");
  const double x_max = rt_x_max(mn);
  for (int64_t t = 0; t < n_traj; ++t) pf_clear(results + t);
  if (n == 0) {  // empty trajectories only: the uniform decision on no rows
    for (int64_t t = 0; t < n_traj; ++t) {
      results[t].anchored = 1;
      results[t].x_uniform = results[t].x_floor = results[t].x_min = x_max;
    }
    return 0;
  }
  if (int rc = h->pf_off.ensure((size_t)n_traj + 1)) return rc;
  StageSpan span(h);
  if (int rc = stage_upload_rows(h, q, qd, qdd, psg, n)) return rc;
  h->pf_hoff.assign(traj_off, traj_off + n_traj + 1);  // (alive until the wait below)
  HIPCHK(hipMemcpyAsync(h->pf_off.p, h->pf_hoff.data(), (size_t)(n_traj + 1) * sizeof(long long),
                        hipMemcpyHostToDevice, h->stream));
  if (int rc2 = pf_enqueue(h, h->rt_in[0].p, h->rt_in[1].p, h->rt_in[2].p,
                           psg ? h->rt_in[3].p : nullptr, n, n_traj, torque_mode, payload_mass, mn,
                           mx))
    return rc2;
  span.end();
  // everything comes back in one wait: the records decide on the host which rows to hand out
  const size_t o_qd = 0, o_qdd = o_qd + (size_t)n * 7, o_psg = o_qdd + (size_t)n * 7,
               o_x = o_psg + (size_t)n, o_u = o_x + (size_t)n, o_ff = o_u + (size_t)n,
               o_end = o_ff + (size_t)n_traj;
  h->pf_host.resize(o_end * sizeof(double));
  double* const hs = reinterpret_cast<double*>(h->pf_host.data());
  if (int rc = stage_download_rows(h, hs + o_qd, hs + o_qdd, hs + o_psg, n)) return rc;
  if (int rc = download(h, hs + o_x, h->pf_x.p, (size_t)n)) return rc;
  if (int rc = download(h, hs + o_u, h->pf_u.p, (size_t)n)) return rc;
  HIPCHK(hipMemcpyAsync(hs + o_ff, h->pf_ff.p, (size_t)n_traj * sizeof(unsigned long long),
                        hipMemcpyDeviceToHost, h->stream));
  if (int rc = download(h, results, h->pf_res.p, (size_t)n_traj)) return rc;
  if (coef_out)
    if (int rc = download(h, coef_out, h->pf_coef.p, (size_t)n * 18)) return rc;
  if (int rc_s = sync_stream(h)) return rc_s;
  const double dt = span.ms();
  if (ms) *ms = dt;
  const unsigned long long* const ff = reinterpret_cast<const unsigned long long*>(hs + o_ff);
  for (int64_t t = 0; t < n_traj; ++t)
    if (results[t].status == kPfBadDelta) return pf_verdict(results + t, 0);
  for (int64_t t = 0; t < n_traj; ++t) {
    tcmp_retime_profile_result& r = results[t];
    (void)pf_verdict(&r, ff[t]);
    r.ms = dt;
    const size_t b = (size_t)traj_off[t], m = (size_t)(traj_off[t + 1] - traj_off[t]);
    if (r.status != TCMP_RETIME_OK || m == 0) continue;
    memcpy(qd_out + 7 * b, hs + o_qd + 7 * b, m * 7 * sizeof(double));
    memcpy(qdd_out + 7 * b, hs + o_qdd + 7 * b, m * 7 * sizeof(double));
    if (psg) memcpy(psg_out + b, hs + o_psg + b, m * sizeof(double));
    if (x_out) memcpy(x_out + b, hs + o_x + b, m * sizeof(double));
    if (u_out) memcpy(u_out + b, hs + o_u + b, m * sizeof(double));
  }
  return 0;
}

int tcmp_plan_retime_profile(tcmp_handle* h, const tcmp_retime_cfg* cfg,
                             tcmp_retime_profile_result* res) {
  TCMP_ENTER(h);
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  double mn, mx;
  if (int rc = rt_cfg(cfg, &mn, &mx)) return rc;
  pf_clear(res);
  const long long K = (long long)h->fin_K;
  if (!stage_applicable(h)) {
    res->status = TCMP_RETIME_NOT_APPLICABLE;
    return 0;
  }
  if (K > 1 && !(h->P.exec_time > 0.0))
    return fail(-1, "psg must ascend strictly inside a trajectory (execution_time is not > 0)");
  if (int rc = h->pf_off.ensure(2)) return rc;
  StageSpan t0(h);
  h->pf_hoff.assign({0, K});  // (alive until the wait below)
  HIPCHK(hipMemcpyAsync(h->pf_off.p, h->pf_hoff.data(), 2 * sizeof(long long), hipMemcpyHostToDevice,
                        h->stream));
  if (int rc = pf_enqueue(h, h->tq.p, h->tqd.p, h->tqdd.p, h->tpsg.p, K, 1, h->P.torque_mode,
                          h->P.mass, mn, mx))
    return rc;
  t0.end();
  unsigned long long ff = 0;
  HIPCHK(hipMemcpyAsync(res, h->pf_res.p, sizeof(*res), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&ff, h->pf_ff.p, sizeof(ff), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  if (int rc = pf_verdict(res, ff)) return rc;
  res->ms = t0.ms();
  if (res->status != TCMP_RETIME_OK) return 0;
  res->exec_time_after = res->time_before != 0.0
                             ? h->P.exec_time * res->time_after / res->time_before
                             : h->P.exec_time;
  StageSpan t1(h);
  if (int rc = plan_commit_rows(h, t1, K, nullptr, h->rt_o[0].p, h->rt_o[1].p, h->rt_o[2].p,
                                nullptr))
    return rc;
  res->ms += t1.ms();
  h->fin_status = -1;  // retimed: not again before the next finish
  return 0;
}

}  // extern "C"
