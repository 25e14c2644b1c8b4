// mxstream — host sanitizer harness. Built by `python -m mxstream.build
// --sanitize` with -fsanitize=address,undefined (and -fno-sanitize-recover) against the C++ twins
// of the kernels, then driven through a few micro-batches of the keyed window pipeline
// (partition -> window_agg -> fire), the vector-metric windows, the window-join twins and the
// table checker, on adversarial shapes: tiny sub-tables, late data, bucket counts at capacity,
// empty batches, unmatched join keys on both ends, every chunking of an expanded pair range.
// Exit code 0 and no sanitizer report = pass (tests/test_debug.py).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "mxs_check.h"
#include "mxs_join.h"
#include "mxs_kernels.h"
#include "mxs_vector.h"

using namespace mxs;

static int fail(const char* what) {
  std::fprintf(stderr, "sanitize_main: %s\n", what);
  return 1;
}

int main() {
  const int64_t n = 20000;
  const int nsub_log2 = 3, cap_log2 = 9, ring = 8, nsub = 1 << nsub_log2, dim = 32;
  const uint32_t bcap = 4096;
  const size_t nslots = (size_t)nsub << cap_log2;
  std::vector<uint64_t> keys(n), vals(n);
  std::vector<int64_t> ts(n);
  std::vector<int32_t> kg_dest(128, 0);
  std::vector<uint32_t> cursor(nsub);
  std::vector<Rec> recs((size_t)nsub * bcap);
  std::vector<int64_t> stats(kStatCount), red(16), local_maxts(1, INT64_MIN);
  std::vector<uint64_t> keys_g(nslots, kEmptyKey), acc_g(ring * nslots);
  std::vector<uint32_t> cnt_g(ring * nslots), occ(nsub), flags(4), late_idx(1024);
  std::vector<uint8_t> dirty_g(ring * nslots);
  std::vector<float> vec((size_t)n * dim), vacc_g(ring * nslots * dim);
  std::vector<uint64_t> vkeys_g(nslots, kEmptyKey);
  std::vector<uint32_t> vcnt_g(ring * nslots);
  std::vector<uint8_t> vdirty_g(ring * nslots);
  std::vector<uint64_t> out_keys(nslots), out_raw(nslots);
  std::vector<double> out_vals(nslots);
  std::vector<float> out_vec(nslots * dim);
  std::vector<uint32_t> out_cnt(nslots), out_n(1);

  int64_t fired_through = INT64_MIN;
  for (int step = 0; step < 6; ++step) {
    const int64_t m = step == 3 ? 0 : n;  // one empty batch
    cpu::gen_events(keys.data(), ts.data(), vals.data(), m, 7, 0, (uint64_t)step * n, 1500,
                    step * 1000, 1000, 400, 0, 1000, 0, 0.0);
    if (step == 5)
      for (int64_t i = 0; i < m; i += 50) ts[i] -= 4000;  // late data
    cpu::gen_vectors(vec.data(), m, dim, 7, 0, (uint64_t)step * n, -10.0f, 100.0f);
    cpu::step_begin(cursor.data(), nsub, stats.data());
    PartPlan pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.max_parallelism = 128;
    pp.nsub_log2 = nsub_log2;
    pp.nranks = 1;
    pp.window_mode = 1;
    pp.drop_late = 1;
    pp.bucket_cap = bcap;
    pp.late_ts = step >= 2 ? (step - 2) * 1000 : INT64_MIN;
    pp.tbase = -1000;
    pp.pane = 500;
    pp.inv_pane = 1.0 / 500;
    pp.rec_words = 3;
    // Values carry the row index for the vector path; the scalar path sums them.
    for (int64_t i = 0; i < m; ++i) vals[i] = (uint64_t)i;
    cpu::partition(keys.data(), ts.data(), vals.data(), nullptr, m, pp, kg_dest.data(),
                   cursor.data(), recs.data(), stats.data(), late_idx.data(),
                   (uint32_t)late_idx.size());
    cpu::step_finish(stats.data(), local_maxts.data(), 400, 1, 0, red.data(), nullptr);
    if (stats[kStatOverflow]) return fail("bucket overflow");
    const int64_t qmin = stats[kStatMinPane], qmax = stats[kStatMaxPane];
    if (qmin > qmax) continue;
    AggPlan ap;
    std::memset(&ap, 0, sizeof(ap));
    ap.cap_log2 = cap_log2;
    ap.nsub = nsub;
    ap.ring = ring;
    ap.agg = AGG_SUM_I64;
    ap.nsrc = 1;
    ap.bucket_cap = bcap;
    ap.np_step = (int32_t)(qmax - qmin + 1);
    ap.pg = 1;
    ap.pane_base = 0;
    ap.p_lo = qmin;
    ap.fired_hi = fired_through;
    ap.rec_words = 3;
    if (ap.np_step > ring) return fail("ring too small");
    cpu::window_agg(recs.data(), cursor.data(), ap, keys_g.data(), acc_g.data(), cnt_g.data(),
                    dirty_g.data(), occ.data(), flags.data());
    VecAggPlan vp;
    std::memset(&vp, 0, sizeof(vp));
    vp.cap_log2 = cap_log2;
    vp.nsub = nsub;
    vp.ring = ring;
    vp.dim = dim;
    vp.nsrc = 1;
    vp.bucket_cap = bcap;
    vp.np_step = ap.np_step;
    vp.rec_words = 3;
    vp.p_lo = qmin;
    vp.fired_hi = fired_through;
    cpu::vec_window_agg(recs.data(), cursor.data(), vp, vec.data(), vkeys_g.data(),
                        vacc_g.data(), vcnt_g.data(), vdirty_g.data(), occ.data(), flags.data());
    // Fire the oldest pane's window (one pane per window here).
    FirePlan fp;
    std::memset(&fp, 0, sizeof(fp));
    fp.agg = AGG_SUM_I64;
    fp.npanes = 1;
    fp.ring = ring;
    fp.nslots = (int64_t)nslots;
    fp.p0 = qmin;
    fp.out_cap = (uint32_t)nslots;
    out_n[0] = 0;
    cpu::window_fire(keys_g.data(), acc_g.data(), cnt_g.data(), dirty_g.data(), fp,
                     out_keys.data(), out_vals.data(), out_raw.data(), out_cnt.data(),
                     out_n.data());
    {
      // Top-N cut of the fired rows (topn_select twin): two windows, the second bound past the
      // capacity (clamped); by raw sum with every column, then by value with the compact
      // layout's null raw / cnt columns and the N smallest.
      std::vector<uint64_t> tk(nslots), tr(nslots);
      std::vector<double> tv(nslots);
      std::vector<uint32_t> tc(nslots), tb(2);
      const uint32_t b2[2] = {out_n[0] / 2, (uint32_t)nslots + 7};
      TopnPlan tp;
      std::memset(&tp, 0, sizeof(tp));
      tp.src = TOP_SRC_I64;
      tp.nwin = 2;
      tp.n = 10;
      tp.cap = (int64_t)nslots;
      const TopnCols in{out_keys.data(), out_vals.data(), out_raw.data(), out_cnt.data()};
      cpu::topn_select(in, b2, tp, TopnCols{tk.data(), tv.data(), tr.data(), tc.data()}, tb.data());
      if (tb[0] < std::min<uint32_t>(10, b2[0]) || tb[1] - tb[0] < 10 || tb[1] > nslots)
        return fail("topn_select: candidate bounds");
      tp.src = TOP_SRC_F64;
      tp.smallest = 1;
      tp.n = 1;
      cpu::topn_select(TopnCols{out_keys.data(), out_vals.data(), nullptr, nullptr}, b2, tp,
                       TopnCols{tk.data(), tv.data(), nullptr, nullptr}, tb.data());
      if (b2[0] && tb[0] < 1) return fail("topn_select: empty cut");
    }
    VecFirePlan vf;
    std::memset(&vf, 0, sizeof(vf));
    vf.dim = dim;
    vf.npanes = 1;
    vf.ring = ring;
    vf.avg = 1;
    vf.nslots = (int64_t)nslots;
    vf.p0 = qmin;
    vf.out_cap = (uint32_t)nslots;
    uint32_t vn = 0;
    cpu::vec_window_fire(vkeys_g.data(), vacc_g.data(), vcnt_g.data(), vdirty_g.data(), vf,
                         out_keys.data(), out_vec.data(), out_cnt.data(), &vn);
    if (vn != out_n[0]) return fail("vector and scalar windows disagree on live keys");
    fired_through = qmin;
  }
  {
    // Sliding count windows (rolling_slide_rows): the pane ring at its 64-pane limit (64, 1), a
    // 65-element pane (130, 65), slide > size (3, 5); two source
    // buckets per sub-table (one full to its capacity), hole records, three batches.
    const int s_nsub = 2, s_cap_log2 = 4, s_nsrc = 2;
    const uint32_t s_bcap = 257;
    const size_t s_slots = (size_t)s_nsub << s_cap_log2;
    const uint32_t shapes[3][2] = {{64, 1}, {130, 65}, {3, 5}};
    for (const auto& sh : shapes) {
      const uint32_t size = sh[0], slide = sh[1], ppw = size / std::gcd(size, slide);
      std::vector<uint64_t> sk(s_slots, kEmptyKey), sa(s_slots), so(s_slots), sr(s_slots * ppw);
      std::vector<uint32_t> sc(s_slots), sflags(4), scount((size_t)s_nsrc * s_nsub);
      std::vector<Rec> srecs((size_t)s_nsrc * s_nsub * s_bcap);
      const uint32_t ocap = 300;  // smaller than the (64, 1) row count: the clamp is exercised
      std::vector<uint64_t> ok(ocap), ov(ocap);
      std::vector<int64_t> ot(ocap);
      std::vector<uint32_t> oc(ocap), on(1);
      uint64_t rows = 0;
      for (int step = 0; step < 3; ++step) {
        for (int b = 0; b < s_nsrc * s_nsub; ++b) {
          const uint32_t c = b == 0 ? s_bcap : 100 + 37 * (uint32_t)b;
          scount[b] = c;
          for (uint32_t e = 0; e < c; ++e) {
            Rec& r = srecs[(size_t)b * s_bcap + e];
            r.key = (uint64_t)(b % s_nsub) * 1000 + e % 5;
            r.val = (uint64_t)(int64_t)((int)e - 50);
            r.t = e % 41 == 40 ? 0xFFFFFFFFu : 0;  // a hole
            r.aux = e;
          }
        }
        on[0] = 0;
        cpu::rolling_slide_rows(srecs.data(), scount.data(), s_nsrc, s_nsub, s_bcap, s_cap_log2,
                                AGG_SUM_I64, sk.data(), sa.data(), sc.data(), so.data(), sr.data(),
                                sflags.data(), ExprProg{}, ok.data(), ov.data(), ot.data(),
                                oc.data(), on.data(), ocap, size, slide);
        rows += on[0];
        for (uint32_t i = 0; i < std::min(on[0], ocap); ++i)
          if (oc[i] < 1 || oc[i] > size) return fail("sliding count window: element count");
      }
      uint64_t total = 0, want = 0;
      for (size_t i = 0; i < s_slots; ++i) {
        total += so[i];
        want += so[i] / slide;
      }
      if (sflags[0] || !total || rows != want) return fail("sliding count window: row count");
    }
  }
  {
    // maxBy / minBy (rolling_arg_rows): rolling and count windows of 1 and 7, the same buckets
    // (one full to its capacity, hole records), an output clamp, three batches. Every winner is a
    // tag of the batch, -1 (the stored record) or, per key only, -2 (an empty open window).
    const int a_nsub = 2, a_cap_log2 = 4, a_nsrc = 2;
    const uint32_t a_bcap = 257, ocap = 300;
    const size_t a_slots = (size_t)a_nsub << a_cap_log2;
    const uint32_t windows[3] = {0, 1, 7};
    for (const uint32_t cw : windows) {
      std::vector<uint64_t> ak(a_slots, kEmptyKey), aa(a_slots);
      std::vector<uint32_t> ac(a_slots), aflags(4), acount((size_t)a_nsrc * a_nsub);
      std::vector<Rec> arecs((size_t)a_nsrc * a_nsub * a_bcap);
      std::vector<uint64_t> ok(ocap), ov(ocap), wk(arecs.size());
      std::vector<int64_t> ot(ocap), os(ocap), ws(arecs.size());
      std::vector<uint32_t> on(1), wn(1);
      for (int step = 0; step < 3; ++step) {
        for (int b = 0; b < a_nsrc * a_nsub; ++b) {
          const uint32_t c = b == 0 ? a_bcap : 100 + 37 * (uint32_t)b;
          acount[b] = c;
          for (uint32_t e = 0; e < c; ++e) {
            Rec& r = arecs[(size_t)b * a_bcap + e];
            r.key = (uint64_t)(b % a_nsub) * 1000 + e % 5;
            r.val = (uint64_t)(int64_t)((int)(e % 4) - step);  // ties everywhere
            r.t = e % 41 == 40 ? 0xFFFFFFFFu : 0;  // a hole
            r.aux = e;
          }
        }
        on[0] = 0;
        cpu::rolling_arg_rows(arecs.data(), acount.data(), a_nsrc, a_nsub, a_bcap, a_cap_log2,
                              AGG_MAX_I64, ak.data(), aa.data(), ac.data(), aflags.data(),
                              ok.data(), ov.data(), ot.data(), os.data(), on.data(), ocap,
                              wk.data(), ws.data(), wn.data(), cw);
        if (wn[0] != 10 || !on[0]) return fail("arg rows: keys touched / rows");
        for (uint32_t i = 0; i < std::min(on[0], ocap); ++i)
          if (os[i] < -1 || (step == 0 && os[i] < 0) || (step > 0 && !cw && os[i] != -1))
            return fail("arg rows: winner of a row");  // (later batches are worse: state wins)
        for (uint32_t i = 0; i < wn[0]; ++i)
          if (ws[i] < -2 || (!cw && step > 0 && ws[i] != -1) || (cw == 1 && ws[i] != -2))
            return fail("arg rows: winner of a key");
      }
      if (aflags[0]) return fail("arg rows: flags");
    }
  }
  {
    // Window join twins (mxs_join.h): matched and unmatched keys on both ends, every pair range
    // of a chunked expand against the nested loop, and a firing without a common key (P = 0).
    const std::vector<int64_t> lk = {1, 3, 4, 5, 9, 10, 12}, ll = {2, 1, 3, 2, 1, 4, 2};
    const std::vector<int64_t> rk = {0, 3, 5, 6, 7, 10, 11}, rl = {1, 2, 3, 1, 1, 2, 5};
    std::vector<int64_t> lh(lk.size()), rh(rk.size());
    int64_t lt = 0, rt = 0;
    for (size_t i = 0; i < lk.size(); ++i) lh[i] = lt, lt += ll[i];
    for (size_t i = 0; i < rk.size(); ++i) rh[i] = rt, rt += rl[i];
    std::vector<uint64_t> lo(lt), ro(rt);
    for (int64_t i = 0; i < lt; ++i) lo[i] = f64_order_bits((uint64_t)(1000 + i));
    for (int64_t i = 0; i < rt; ++i) ro[i] = f64_order_bits((uint64_t)(2000 + i));
    const JoinSide L{lk.data(), lh.data(), (int64_t)lk.size(), lt};
    const JoinSide R{rk.data(), rh.data(), (int64_t)rk.size(), rt};
    const int64_t kl = L.nseg;
    std::vector<int64_t> match(kl), off(kl + 1), plan(kJoinPlanCols * (kl + 1)), meta(kJoinMeta);
    std::vector<uint64_t> cnt(kl);
    cpu::join_match(L, R, match.data(), cnt.data());
    cpu::join_scan(L, R, match.data(), cnt.data(), off.data(), plan.data(), meta.data());
    std::vector<int64_t> want;  // the nested loop: (key, left, right) rows
    for (int64_t i = 0; i < kl; ++i)
      for (size_t j = 0; j < rk.size(); ++j)
        if (rk[j] == lk[i])
          for (int64_t a = 0; a < ll[i]; ++a)
            for (int64_t b = 0; b < rl[j]; ++b) {
              want.push_back(lk[i]);
              want.push_back(1000 + lh[i] + a);
              want.push_back(2000 + rh[j] + b);
            }
    const int64_t P = meta[kJoinP];
    if (P != (int64_t)want.size() / 3 || P != 16 || meta[kJoinM] != 3 || meta[kJoinErr] ||
        match[0] != -1 || match[kl - 1] != -1 || off[kl] != P)
      return fail("join: match / scan");
    for (int64_t chunk = 1; chunk <= P + 1; ++chunk)
      for (int64_t p0 = 0; p0 < P; p0 += chunk) {
        const int64_t p1 = std::min(P, p0 + chunk), m = p1 - p0;
        std::vector<int64_t> ok(m), ol(m), orr(m);  // exactly the range: a write past it is caught
        cpu::join_expand(L, R, match.data(), off.data(), lo.data(), ro.data(), p0, p1, ok.data(),
                         ol.data(), orr.data());
        for (int64_t p = p0; p < p1; ++p)
          if (ok[p - p0] != want[3 * p] || ol[p - p0] != want[3 * p + 1] ||
              orr[p - p0] != want[3 * p + 2])
            return fail("join: expanded range");
      }
    const std::vector<int64_t> ok2 = {2, 8}, oh2 = {0, 1};
    const JoinSide R2{ok2.data(), oh2.data(), 2, 2}, E{nullptr, nullptr, 0, 0};
    cpu::join_match(L, R2, match.data(), cnt.data());
    cpu::join_scan(L, R2, match.data(), cnt.data(), off.data(), plan.data(), meta.data());
    if (meta[kJoinP] != 0 || meta[kJoinM] != 0 || off[kl] != 0) return fail("join: P = 0");
    cpu::join_expand(L, R2, match.data(), off.data(), lo.data(), ro.data(), 0, 0, nullptr, nullptr,
                     nullptr);
    cpu::join_match(E, R, nullptr, nullptr);
    cpu::join_scan(E, R, nullptr, nullptr, off.data(), plan.data(), meta.data());
    if (meta[kJoinP] != 0 || off[0] != 0) return fail("join: empty side");
  }
  uint64_t chk[kChkN] = {0, 0, 0, 0};
  cpu::check_table(keys_g.data(), nsub, nsub_log2, cap_log2, chk);
  if (chk[kChkMisplaced] || chk[kChkBrokenChain] || chk[kChkDuplicate] || !chk[kChkLive])
    return fail("table invariant violated");
  std::printf("sanitize_main ok: %llu live keys\n", (unsigned long long)chk[kChkLive]);
  return 0;
}
