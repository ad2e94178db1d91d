// tcmp_stage.h -- what the opt-in stages on a finished trajectory share (tcmp_retime.h,
// tcmp_retime_runs.h, tcmp_retime_profile.h, tcmp_repair.h; the span guard also tcmp_shortcut.h
// and tcmp_goal.h).  The engine's results are compared byte for byte, so every rule that more than
// one stage applies is stated here once: a joint's interval in x, the decision from a reduced
// interval, the tail of the row kernels, the plan's commit.  The stage headers keep their own
// arithmetic and call these.
#pragma once

namespace {

constexpr double kRtEps = 1e-9;  // guard on the limit: the tolerance the RNE is pinned at

// ---- device ---------------------------------------------------------------------------------

// The interval [l, u] of x = 1 / s^2 in which one joint passes the torque test: its torque is
// g + x d against the limit L (include/tcmp.h states the rule; tests/retime_ref.py is the
// oracle).  d == 0: every x or none, by the static torque alone.  A NaN torque proves nothing:
// the empty interval, so u is never NaN.
__device__ __forceinline__ void rt_interval(double g, double d, double L, double& u, double& l) {
#pragma clang fp contract(off)
  const double Lg = L - kRtEps;
  if (d != 0.0) {
    const double ad = fabs(d), sg = d > 0.0 ? g : -g;
    u = (Lg - sg) / ad;
    l = (-Lg - sg) / ad;
  } else if (fabs(g) < L) {
    u = INFINITY;
    l = 0.0;
  } else {
    u = -INFINITY;
    l = INFINITY;
  }
  if (!(u == u) || !(l == l)) {
    u = -INFINITY;
    l = INFINITY;
  }
}

// The decision from a reduced interval [x_lo, x_hi]: the largest x up to x_max = 1 / min_scale^2
// (snap, min_scale == 1: never faster than given, and x = 1 keeps every bit), INFEASIBLE when
// that is not in the interval, OVER_CAP when it is below x_cap = 1 / max_scale^2 (capped:
// max_scale > 0).  The callers divide; nothing here rounds.  fmin on the host and the device
// alike: it differs from std::min only on a NaN, and x_hi is never one (rt_interval).
struct RtDecision {
  int status;
  double x;  // meaningful when status is TCMP_RETIME_OK
};
__host__ __device__ __forceinline__ RtDecision rt_decide(double x_hi, double x_lo, double x_max,
                                                         double x_cap, bool snap, bool capped) {
  double x = fmin(x_max, x_hi);
  if (x >= 1.0 && snap) x = 1.0;
  const int status = (!(x > 0.0) || x < x_lo) ? TCMP_RETIME_INFEASIBLE
                     : (capped && x < x_cap)   ? TCMP_RETIME_OVER_CAP
                                               : TCMP_RETIME_OK;
  return RtDecision{status, x};
}

// the tail of an apply kernel: row i's new rates to oqd / oqdd, then the mode's torque test on
// (c, v, a); a failing row lowers *slot to val
template <int MODE>
__device__ __forceinline__ void stage_store_test(const double c[7], const double v[7],
                                                 const double a[7], double mass, long long i,
                                                 double* oqd, double* oqdd,
                                                 unsigned long long* slot,
                                                 unsigned long long val) {
  double cq[7], sq[7];
  store7(oqd + 7 * i, v);
  store7(oqdd + 7 * i, a);
  sincos7(c, cq, sq);
  if (!torque_test_m<MODE>(mass, cq, sq, v, a)) atomicMin(slot, val);
}

// the k with off[k] <= i < off[k + 1] among n_off intervals (off[0] = 0 <= i < off[n_off]; equal
// offsets, an empty interval, go to the successor)
__device__ __forceinline__ long long stage_find(const long long* __restrict__ off, long long n_off,
                                                long long i) {
  long long lo = 0, hi = n_off;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the plan's stored verdict on new rows: their first failing row (null: a stage that verified)
__global__ void k_stage_commit(DevState* st, const unsigned long long* first_fail) {
  const unsigned long long ff = first_fail ? *first_fail : kNoRow;
  st->status = ff == kNoRow ? TCMP_PLAN_OK : TCMP_PLAN_VALIDATION_FAILED;
  st->first_fail = ff == kNoRow ? -1 : (long long)ff;
}

// ---- host -----------------------------------------------------------------------------------

// A timed span of the handle's stream: a mark at construction, one at end(), and both back in
// the pool on every way out of the scope (only a plan finish's collect_events recycles marks,
// and a stand-alone call may never see one).  ms() is valid once the stream has passed end().
class StageSpan {
 public:
  explicit StageSpan(tcmp_handle* h) : h_(h), a_(h->mark()) {}
  StageSpan(const StageSpan&) = delete;
  StageSpan& operator=(const StageSpan&) = delete;
  ~StageSpan() {
    for (hipEvent_t e : {a_, b_}) {
      const auto it = std::find(h_->ev_rec.begin(), h_->ev_rec.end(), e);
      if (e && it != h_->ev_rec.end()) {
        h_->ev_rec.erase(it);
        h_->ev_pool.push_back(e);
      }
    }
  }
  void end() { b_ = h_->mark(); }
  bool timed() const { return a_ && b_; }  // false with timing off (tcmp_set_timing)
  float ms() const {
    float t = 0;
    return timed() && hipEventElapsedTime(&t, a_, b_) == hipSuccess ? t : 0.f;
  }

 private:
  tcmp_handle* h_;
  hipEvent_t a_, b_ = nullptr;
};

// may a stage work on the rows of the plan's last finish
bool stage_applicable(const tcmp_handle* h) {
  return (h->fin_status == TCMP_PLAN_OK || h->fin_status == TCMP_PLAN_VALIDATION_FAILED) &&
         (long long)h->fin_K > 0;
}

// the stand-alone forms' rows in: the caller's q, qd, qdd (n rows of 7) and psg (n or null)
// into h->rt_in[0..3] ...
int stage_upload_rows(tcmp_handle* h, const double* q, const double* qd, const double* qdd,
                      const double* psg, long long n) {
  int rc = psg ? 0 : h->rt_in[3].ensure((size_t)n);
  const double* src[3] = {q, qd, qdd};
  for (int k = 0; k < 3; ++k) rc = rc ? rc : upload(h, h->rt_in[k], src[k], (size_t)n * 7);
  if (psg) rc = rc ? rc : upload(h, h->rt_in[3], psg, (size_t)n);
  return rc;
}

// ... and out: h->rt_o[0..2] into the caller's (psg: null to leave it out).  Enqueued only.
int stage_download_rows(tcmp_handle* h, double* qd, double* qdd, double* psg, long long n) {
  if (int rc = download(h, qd, h->rt_o[0].p, (size_t)n * 7)) return rc;
  if (int rc = download(h, qdd, h->rt_o[1].p, (size_t)n * 7)) return rc;
  if (psg)
    if (int rc = download(h, psg, h->rt_o[2].p, (size_t)n)) return rc;
  return 0;
}

// A stage's K new rows into the open plan's (q, psg: null to keep the plan's), Conf.torques of
// the new rows, the stored verdict -- first_fail: the device word holding the new rows' first
// failing row, null for rows their stage verified -- and, after a wait, the pinned copy of it.
// t: the caller's running span, ended here; t.ms() is valid on return.
int plan_commit_rows(tcmp_handle* h, StageSpan& t, long long K, const double* q, const double* qd,
                     const double* qdd, const double* psg, const unsigned long long* first_fail) {
  const size_t nb = (size_t)K * 7 * sizeof(double);
  if (q) HIPCHK(hipMemcpyAsync(h->tq.p, q, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tqd.p, qd, nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tqdd.p, qdd, nb, hipMemcpyDeviceToDevice, h->stream));
  if (psg)
    HIPCHK(hipMemcpyAsync(h->tpsg.p, psg, (size_t)K * sizeof(double), hipMemcpyDeviceToDevice,
                          h->stream));
  // (the state still holds the finish's K and status)
  hipLaunchKernelGGL(k_traj_tau, dim3(grid_for(K, 256)), dim3(256), 0, h->stream, h->st, h->tq.p,
                     h->tqd.p, h->tqdd.p, h->ttau.p, h->kcap);
  hipLaunchKernelGGL(k_stage_commit, dim3(1), dim3(1), 0, h->stream, h->st, first_fail);
  HIPCHK(hipGetLastError());
  t.end();
  unsigned long long ff = kNoRow;
  if (first_fail)
    HIPCHK(hipMemcpyAsync(&ff, first_fail, sizeof(ff), hipMemcpyDeviceToHost, h->stream));
  if (int rc_s = sync_stream(h)) return rc_s;
  h->pin()->st.status = ff == kNoRow ? TCMP_PLAN_OK : TCMP_PLAN_VALIDATION_FAILED;
  h->pin()->st.first_fail = ff == kNoRow ? -1 : (long long)ff;
  return 0;
}

}  // namespace
