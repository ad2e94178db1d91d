// tcmp_repair.h -- collision repair of the min-jerk trajectory (tcmp_repair_traj,
// tcmp_plan_repair): an opt-in stage between the finish and the retiming.  k_edges checks the
// chords between waypoints; the min-jerk rows leave them, because every joint of an interior
// waypoint gets its own velocity (gv_at) and so its own time profile inside a segment.  The stage
// runs collision_fn on the rows and, where one fails, zeroes the velocities of the two waypoints
// of its segment ("closes their gates"): between two closed gates all seven joints share the
// rest-to-rest profile 10 t^3 - 15 t^4 + 6 t^5 and the rows lie on the checked chord.  A segment's
// rows depend on its own two gates only, so a pass samples just the segments next to a gate the
// pass before closed (include/tcmp.h states the passes; DESIGN §3 restates them;
// tests/repair_ref.py is the oracle).
//
// Per pass k_repair_rows (one row per lane: gated min-jerk sample, collision_fn, the segment's
// first failing row and failing count by integer atomics) and k_repair_update (one block: the
// verdict, the gates, the next dirty list, the summary the host reads); the next pass's grid
// depends on the summary, so there is one host wait per pass, and at most W - 1 passes.
#pragma once

namespace {

// a pass's summary (device copy in rp_sum, then the handle's pinned block)
struct RpSum {
  int state;               // 0: some segment hit, none stuck; 1: no segment hit; 2: one is stuck
  int n_dirty;             // segments of the next pass (state 0 with gates to close)
  long long first_hit;     // lowest failing row over all segments, -1: none
  long long rows_hit;      // failing rows over all segments
  long long gates_closed;  // by this pass
  long long stuck_seg, stuck_row;  // state 2: the lowest stuck segment and its first failing row
};

// every gate open, every segment dirty
__global__ __launch_bounds__(256) void k_repair_init(long long W, int* g0, int* g1, int* dirty,
                                                     unsigned long long* first, unsigned* count) {
  for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < W;
       w += (long long)gridDim.x * 256) {
    g0[w] = 1;
    g1[w] = 1;
    if (w < W - 1) {
      dirty[w] = (int)w;
      first[w] = kNoRow;
      count[w] = 0u;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_repair_rows: lane r of the compacted rows takes row j = r % ni of segment dirty[r / ni]
// (ni is arbitrary: waves and blocks straddle segments).  Lanes past the end stay in the wave
// for collides_wave, at the joint ranges' middle, as in k_check_configs.
// ------------------------------------------------------------------------------------------
template <bool MESH>
__global__ __launch_bounds__(256) void k_repair_rows(const double* wp, long long W, long long ni,
                                                     const int* gates, const int* dirty,
                                                     long long n_rows, Scene sc_g, Geo g_g,
                                                     double* oq, double* oqd, double* oqdd,
                                                     unsigned long long* first, unsigned* count) {
  extern __shared__ double tcmp_lds[];
  Scene sc;
  Geo g;
  stage_lds<!MESH>(sc_g, g_g, tcmp_lds, sc, g);
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool act = r < n_rows;
  long long s = 0, i = 0;
  double x[7];
  if (act) {
    s = dirty[r / ni];
    i = s * ni + r % ni;
    double v[7], a[7];
    minjerk_sample(wp, W, ni, i, x, v, a, gates);
    store7(oq + 7 * i, x);
    store7(oqd + 7 * i, v);
    store7(oqdd + 7 * i, a);
  } else {
    for (int k = 0; k < 7; ++k) x[k] = 0.5 * (kLo[k] + kHi[k]);
  }
  double cq[7], sq[7];
  for (int k = 0; k < 7; ++k) sincos(x[k], &sq[k], &cq[k]);
  StepStats ss = {0, 0, 0};
  const bool lim = act && limits_violated(x);
  const bool c = collides_wave<MESH>(cq, sq, act && !lim, sc, g, ss) || lim;
  if (act && c) {
    atomicMin(first + s, (unsigned long long)i);
    atomicAdd(count + s, 1u);
  }
}

// ------------------------------------------------------------------------------------------
// k_repair_update: one block, a thread per segment (strided).  A segment's count is its last
// check's (a clean segment was not hit, or the passes would have ended).  Gates are read from
// gi and written to go, so no thread reads what another writes before a barrier; every sum and
// minimum is an integer's.  One workgroup on one CU, 20 barriers of scan per 1,024 segments:
// right for a planner's paths (under 10^4 waypoints, microseconds), serial for a list of
// millions, which tcmp_repair_traj accepts but is not built for.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_repair_update(long long W, const int* gi, int* go,
                                                        unsigned long long* first,
                                                        unsigned* count, int* dirty,
                                                        int may_close, RpSum* out) {
  __shared__ unsigned long long s_first, s_rows, s_stuck, s_closed;
  __shared__ int s_scan[1024];
  const int tid = threadIdx.x;
  const long long nseg = W - 1;
  if (tid == 0) {
    s_first = kNoRow;
    s_rows = 0;
    s_stuck = kNoRow;
    s_closed = 0;
  }
  __syncthreads();
  {
    unsigned long long f = kNoRow, n = 0, stuck = kNoRow;
    for (long long s = tid; s < nseg; s += 1024) {
      const unsigned c = count[s];
      if (!c) continue;
      n += c;
      const unsigned long long fs = first[s];
      f = fs < f ? fs : f;
      const bool open0 = s > 0 && gi[s] != 0, open1 = s + 1 < nseg && gi[s + 1] != 0;
      if (!open0 && !open1 && (unsigned long long)s < stuck) stuck = (unsigned long long)s;
    }
    if (n) {
      atomicMin(&s_first, f);
      atomicAdd(&s_rows, n);
    }
    if (stuck != kNoRow) atomicMin(&s_stuck, stuck);
  }
  __syncthreads();
  const unsigned long long rows = s_rows, stuck = s_stuck;
  const int state = rows == 0 ? 1 : stuck != kNoRow ? 2 : 0;
  const bool close = state == 0 && may_close;
  long long run = 0;
  if (close) {
    unsigned long long closed = 0;
    for (long long w = tid; w < W; w += 1024) {
      int gw = gi[w];
      if (w > 0 && w < nseg && gw != 0 && (count[w - 1] != 0u || count[w] != 0u)) {
        gw = 0;
        ++closed;
      }
      go[w] = gw;
    }
    if (closed) atomicAdd(&s_closed, closed);
    __syncthreads();
    // the segments next to a gate that changed, in order (a block scan per 1024 segments)
    for (long long b0 = 0; b0 < nseg; b0 += 1024) {
      const long long s = b0 + tid;
      const int flag = s < nseg && (gi[s] != go[s] || gi[s + 1] != go[s + 1]) ? 1 : 0;
      s_scan[tid] = flag;
      __syncthreads();
      for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
      }
      if (flag) {
        dirty[run + s_scan[tid] - 1] = (int)s;
        first[s] = kNoRow;
        count[s] = 0u;
      }
      run += s_scan[1023];
      __syncthreads();
    }
  }
  if (tid == 0) {
    RpSum r;
    r.state = state;
    r.n_dirty = (int)run;
    r.first_hit = rows ? (long long)s_first : -1;
    r.rows_hit = (long long)rows;
    r.gates_closed = (long long)s_closed;
    r.stuck_seg = state == 2 ? (long long)stuck : -1;
    r.stuck_row = state == 2 ? (long long)first[stuck] : -1;
    *out = r;
  }
}

int rp_cfg(const tcmp_repair_cfg* cfg, int* max_passes, int* check_only) {
  *max_passes = cfg ? cfg->max_passes : 0;
  *check_only = cfg && cfg->check_only ? 1 : 0;
  if (*max_passes < 0) return fail(-1, "max_passes below 0");
  return 0;
}

void rp_clear(tcmp_repair_result* r) {
  memset(r, 0, sizeof(*r));
  r->first_hit_before = r->first_hit_after = -1;
  r->stuck_segment = r->stuck_row = -1;
  r->first_fail_before = r->first_fail_after = -1;
}

// The passes on W >= 2 device waypoints (rows of 7), ni >= 1: the rows of the final gates are in
// h->rp_o[0..2] and the gates in h->rp_gate[*gcur] when the status is OK.  The waypoints are only
// read.  One host wait per pass.
int rp_passes(tcmp_handle* h, const double* wp, long long W, long long ni, int max_passes,
              int check_only, tcmp_repair_result* r, int* gcur) {
  const long long nseg = W - 1, K = nseg * ni;
  int rc = 0;
  for (int k = 0; k < 3; ++k) rc = rc ? rc : h->rp_o[k].ensure((size_t)K * 7);
  for (int k = 0; k < 2; ++k) rc = rc ? rc : h->rp_gate[k].ensure((size_t)W);
  rc = rc ? rc : h->rp_dirty.ensure((size_t)nseg);
  rc = rc ? rc : h->rp_first.ensure((size_t)nseg);
  rc = rc ? rc : h->rp_count.ensure((size_t)nseg);
  rc = rc ? rc : h->rp_sum.ensure(sizeof(RpSum));
  if (rc) return rc;
  if (int rc = h->rp_pin.ensure(sizeof(RpSum))) return rc;
  RpSum* const dsum = reinterpret_cast<RpSum*>(h->rp_sum.p);
  const RpSum& s = *static_cast<const RpSum*>(h->rp_pin.p);
  const bool mk = h->mesh_kernels();
  hipLaunchKernelGGL(k_repair_init, dim3(std::min<unsigned>(grid_for(W, 256), 1024)), dim3(256), 0,
                     h->stream, W, h->rp_gate[0].p, h->rp_gate[1].p, h->rp_dirty.p, h->rp_first.p,
                     h->rp_count.p);
  int cur = 0;
  long long n_dirty = nseg;
  for (int pass = 1;; ++pass) {
    const long long rows = n_dirty * ni;
    hipLaunchKernelGGL(mk ? k_repair_rows<true> : k_repair_rows<false>, dim3(grid_for(rows, 256)),
                       dim3(256), lds_bytes(h), h->stream, wp, W, ni, h->rp_gate[cur].p,
                       h->rp_dirty.p, rows, h->scene(), h->geo(), h->rp_o[0].p, h->rp_o[1].p,
                       h->rp_o[2].p, h->rp_first.p, h->rp_count.p);
    const int may_close = !check_only && !(max_passes > 0 && pass >= max_passes);
    hipLaunchKernelGGL(k_repair_update, dim3(1), dim3(1024), 0, h->stream, W, h->rp_gate[cur].p,
                       h->rp_gate[cur ^ 1].p, h->rp_first.p, h->rp_count.p, h->rp_dirty.p,
                       may_close, dsum);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->rp_pin.p, dsum, sizeof(RpSum), hipMemcpyDeviceToHost, h->stream));
    if (int rc_s = sync_stream(h)) return rc_s;
    r->passes_run = pass;
    r->segments_resampled += n_dirty;
    r->rows_checked += rows;
    if (pass == 1) {
      r->first_hit_before = s.first_hit;
      r->rows_hit_before = s.rows_hit;
    }
    r->first_hit_after = s.first_hit;
    r->rows_hit_after = s.rows_hit;
    if (s.state == 1) {
      r->status = TCMP_REPAIR_OK;
      break;
    }
    if (check_only) {
      r->status = TCMP_REPAIR_COLLIDES;
      break;
    }
    if (s.state == 2) {
      r->status = TCMP_REPAIR_UNRESOLVED;
      r->stuck_segment = s.stuck_seg;
      r->stuck_row = s.stuck_row;
      break;
    }
    if (!may_close) {
      r->status = TCMP_REPAIR_PASS_CAP;
      break;
    }
    // a hit segment that is not stuck has an open gate, so the pass closed one
    if (s.gates_closed <= 0 || s.n_dirty <= 0) return fail(-5, "repair pass closed no gate");
    r->gates_closed += s.gates_closed;
    cur ^= 1;
    n_dirty = s.n_dirty;
  }
  *gcur = cur;
  return 0;
}

// rp_passes between two marks
int rp_run(tcmp_handle* h, const double* wp, long long W, long long ni, int max_passes,
           int check_only, tcmp_repair_result* r, int* gcur) {
  rp_clear(r);
  r->n_rows = (W - 1) * ni;
  r->n_segments = W - 1;
  StageSpan t(h);
  if (int rc = rp_passes(h, wp, W, ni, max_passes, check_only, r, gcur)) return rc;
  t.end();
  if (t.timed()) {
    if (int rc_s = sync_stream(h)) return rc_s;
    r->ms = t.ms();
  }
  return 0;
}

}  // namespace

namespace {
// dynamic LDS above 64 KiB per workgroup must be allowed explicitly (tcmp_create)
int repair_lds_limits() {
  const int lim = (int)stage_lds_bytes(kMaxObstacles);
  for (const void* k : {(const void*)k_repair_rows<false>, (const void*)k_repair_rows<true>})
    HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lim));
  return 0;
}
}  // namespace

extern "C" {

int tcmp_repair_traj(tcmp_handle* h, const double* waypoints, int64_t n_wp, int64_t ni,
                     const tcmp_repair_cfg* cfg, double* q, double* qd, double* qdd, int32_t* gates,
                     tcmp_repair_result* res) {
  TCMP_ENTER(h);
  if (int rc = att_refuse(h, "tcmp_repair_traj")) return rc;
  if (!res || !waypoints) return fail(-1, "bad arguments");
  if (n_wp < 2) return fail(-1, "fewer than two waypoints");
  if (ni < 1) return fail(-1, "Invalid number of intervals chosen (must be greater than 0)");
  if (n_wp > INT_MAX || ni > INT_MAX || (n_wp - 1) * ni > (1ll << 38))
    return fail(-1, "trajectory too long");
  int max_passes, check_only;
  if (int rc = rp_cfg(cfg, &max_passes, &check_only)) return rc;
  if (!check_only && (!q || !qd || !qdd || !gates)) return fail(-1, "bad arguments");
  if (int rc = upload(h, h->rp_wp, waypoints, (size_t)n_wp * 7)) return rc;
  int cur = 0;
  if (int rc = rp_run(h, h->rp_wp.p, n_wp, ni, max_passes, check_only, res, &cur)) return rc;
  if (res->status != TCMP_REPAIR_OK || check_only) return 0;
  double* const rows[3] = {q, qd, qdd};
  for (int k = 0; k < 3; ++k)
    if (int rc = download(h, rows[k], h->rp_o[k].p, (size_t)res->n_rows * 7)) return rc;
  if (int rc = download(h, gates, h->rp_gate[cur].p, (size_t)n_wp)) return rc;
  return sync_stream(h);
}

int tcmp_plan_repair(tcmp_handle* h, const tcmp_repair_cfg* cfg, tcmp_repair_result* res) {
  TCMP_ENTER(h);
  if (int rc = att_refuse(h, "tcmp_plan_repair")) return rc;
  if (!res) return fail(-1, "null result");
  if (!h->plan_open) return fail(-1, "no open plan");
  int max_passes, check_only;
  if (int rc = rp_cfg(cfg, &max_passes, &check_only)) return rc;
  rp_clear(res);
  const long long W = (long long)h->fin_W, K = (long long)h->fin_K;
  if (!stage_applicable(h) || h->repaired || W < 2) {
    res->status = TCMP_REPAIR_NOT_APPLICABLE;
    return 0;
  }
  const long long ni = K / (W - 1);  // K = (W - 1) ni (k_retrace's tail)
  int cur = 0;
  if (int rc = rp_run(h, h->wp.p, W, ni, max_passes, check_only, res, &cur)) return rc;
  res->first_fail_before = res->first_fail_after = h->fin_first_fail;
  if (res->status != TCMP_REPAIR_OK || check_only) return 0;
  if (res->gates_closed == 0) {  // the rows are the finish's own: nothing to replace
    h->repaired = true;
    return 0;
  }
  if (int rc = h->u0.ensure(1)) return rc;
  if (int rc = h->pl_gate.ensure((size_t)W)) return rc;
  // From here the engine's rows change: an error on the way leaves the plan with neither a
  // repair nor a retiming applicable until its next finish.
  h->fin_status = -1;
  StageSpan t(h);
  // the plan's own copy of the gates (tcmp_plan_retime_runs derives its runs from them; a
  // later stand-alone tcmp_repair_traj on this handle overwrites rp_gate)
  HIPCHK(hipMemcpyAsync(h->pl_gate.p, h->rp_gate[cur].p, (size_t)W * sizeof(int),
                        hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->u0.p, 0xff, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(TCMP_BY_MODE(k_validate, h->P.torque_mode, 7), dim3(grid_for(K, 256)),
                     dim3(256), 0, h->stream, h->rp_o[0].p, h->rp_o[1].p, h->rp_o[2].p, K,
                     h->P.mass, h->u0.p);
  if (int rc = plan_commit_rows(h, t, K, h->rp_o[0].p, h->rp_o[1].p, h->rp_o[2].p, nullptr,
                                h->u0.p))
    return rc;
  res->ms += t.ms();
  res->first_fail_after = h->pin()->st.first_fail;
  h->fin_status = h->pin()->st.status;
  h->fin_first_fail = res->first_fail_after;
  h->repaired = true;
  h->pl_gated = true;
  return 0;
}

}  // extern "C"
