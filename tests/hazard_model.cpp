// CPU test of the packet-buffer hazard checker (swraytracing_amd/csrc/
// swrt_hazard.hpp): replays the multi-stream launch protocol of the library
// (swrt_host_packets.hpp tile_launch / launch_tiles / rebin, swrt_ctx.hpp
// join_b) in the abstract — buffers are
// tags, launches are accesses over the band slots the device mapping gives
// each part (swrt_share.hpp share_slot, the same function the kernels run)
// — and prints one line per scenario: "<name> ok" when the checker's verdict
// is the expected one.  The rotation of the three packet sets is the library's
// own (swrt_packet_state.hpp SetRing), and the last blocks drive its Binning
// and its SeriesExtent (the frame series' counting) through the transitions
// the library makes.  Built (hipcc, host code only) and run by
// tests/test_hazard_model.py; no GPU.
#include <cstdio>
#include <string>
#include <vector>

#include "../swraytracing_amd/csrc/swrt_hazard.hpp"
#include "../swraytracing_amd/csrc/swrt_packet_state.hpp"

using namespace swrt;

namespace {

struct Proto {
  HazardChecker h;
  SetRing<int> pk{0, 1, 2};  // the three packet sets (one tag stands for x, k, perm)
  int src = 10, counts = 11, fork = 20, join[3] = {21, 22, 23};
  int pending = 0;
  bool legacy = false;
  int ntiles = 64;  // 8 XCD bands x 8 band positions
  const void* B(int i) { return reinterpret_cast<const void*>(static_cast<intptr_t>(0x1000 + 16 * i)); }

  bool join_b() {
    for (int i = 0; i < pending; ++i) {
      h.record(B(join[i]), i + 1);
      h.wait(0, B(join[i]));
    }
    pending = 0;
    return true;
  }
  // re-binning on the packet stream (indirect: only the source index)
  bool rebin(bool do_join = true) {
    if (do_join) join_b();
    const uint64_t t = h.op(0);
    bool ok = h.access(0, t, B(pk.cur), kHzRead, HzRegion::all(), "rebin") &&
              h.access(0, t, B(counts), kHzWrite, HzRegion::all(), "rebin") &&
              h.access(0, t, B(src), kHzWrite, HzRegion::all(), "rebin");
    ++h.epoch;
    return ok;
  }
  // one tile launch as S parts (share rule `rule`); sort = the first launch
  // after a re-binning
  bool launch(int S, bool sort, bool count_next = false, int rule = kShareEven) {
    if (S > 1) {
      h.record(B(fork), 0);
      for (int i = 1; i < S; ++i) h.wait(i, B(fork));
    }
    for (int p = 0; p < S; ++p) {
      const uint64_t t = h.op(p);
      const HzRegion r = HzRegion::of_share(h.epoch, S > 1 ? TileShare{ntiles, p, S, rule} : TileShare{ntiles, -1, 1, 0});
      bool ok = h.access(p, t, B(pk.cur), kHzRead, sort ? HzRegion::all() : r, "part") &&
                (!sort || h.access(p, t, B(src), kHzRead, r, "part")) &&
                h.access(p, t, B(pk.out), kHzWrite, r, "part") &&
                (!count_next || h.access(p, t, B(counts), kHzAtomic, HzRegion::all(), "part"));
      if (!ok) return false;
    }
    pending = S - 1;
    if (sort && pending && !legacy) pk.park_cur();  // park the gathered-from buffer
    else pk.flip();
    return true;
  }
  // a per-packet launch over every packet on the packet stream
  bool whole(bool do_join) {
    if (do_join) join_b();
    const uint64_t t = h.op(0);
    return h.access(0, t, B(pk.cur), kHzWrite, HzRegion::all(), "whole launch");
  }
};

int fails = 0;
void expect(const char* name, bool got, bool want, const Proto& p = Proto()) {
  if (got == want) {
    std::printf("%s ok\n", name);
  } else {
    std::printf("%s FAILED (checker %s)%s%s\n", name, got ? "silent" : "reported", got ? "" : ": ",
                got ? "" : p.h.err.c_str());
    ++fails;
  }
}

}  // namespace

int main() {
  {  // the shared mapping: every slot taken exactly once by the parts of a launch, for both rules
    bool ok = true;
    for (int rule : {kShareEven, kShareSkew})
      for (int nt : {64, 72, 1024}) {
        if (rule == kShareEven && nt % 16) continue;  // the library splits evenly only when 16 | ntiles
        std::vector<int> seen(nt, 0);
        for (int p = 0; p < 2; ++p) {
          const TileShare sh{nt, p, 2, rule};
          for (int b = 0; b < share_grid(sh); ++b) ++seen[share_slot(sh, b)];
        }
        for (int v : seen) ok = ok && v == 1;
      }
    std::vector<int> all(100, 0);
    for (int b = 0; b < 100; ++b) ++all[share_slot(TileShare{100, -1, 1, 0}, b)];
    for (int v : all) ok = ok && v == 1;
    expect("share_partitions_slots", ok, true, Proto());
  }
  {  // round 4's hang: the cycle-ending launch takes a skewed share -> reported
    Proto p;
    bool ok = p.rebin();
    for (int l = 0; l < 3 && ok; ++l) ok = p.launch(2, l == 0);
    expect("even_launches_silent", ok, true, p);
    ok = p.launch(2, false, true, kShareSkew);
    expect("skewed_cycle_end_reported", ok, false, p);
    std::printf("  message: %s\n", p.h.err.c_str());
  }
  {  // a skewed share used by every launch of a binning is a consistent mapping: silent
    Proto p;
    bool ok = true;
    for (int cyc = 0; cyc < 2 && ok; ++cyc) {
      ok = ok && p.rebin();
      for (int l = 0; l < 4 && ok; ++l) ok = p.launch(2, l == 0, l == 3, kShareSkew);
    }
    expect("consistent_skew_silent", ok, true, p);
  }
  for (int S : {2}) {
    const std::string sfx = "_s" + std::to_string(S);
    {  // the library's protocol over three re-binning cycles: silent
      Proto p;
      bool ok = true;
      for (int cyc = 0; cyc < 3 && ok; ++cyc) {
        ok = ok && p.rebin();
        for (int l = 0; l < 4 && ok; ++l) ok = p.launch(S, l == 0, l == 3);
      }
      expect(("protocol_third_buffer" + sfx).c_str(), ok, true, p);
    }
    {  // legacy ordering: the launch after the sort launch is reported
      Proto p;
      p.legacy = true;
      bool ok = p.rebin() && p.launch(S, true);
      expect(("sort_launch_parts_ok" + sfx).c_str(), ok, true, p);
      ok = p.launch(S, false);
      expect(("legacy_park_reported" + sfx).c_str(), ok, false, p);
      std::printf("  message: %s\n", p.h.err.c_str());
    }
    {  // a whole launch after split calls must join first
      Proto p;
      bool ok = p.rebin() && p.launch(S, true) && p.launch(S, false);
      expect(("split_calls" + sfx).c_str(), ok, true, p);
      Proto q = p;
      expect(("whole_launch_without_join_reported" + sfx).c_str(), q.whole(false), false, q);
      expect(("whole_launch_after_join" + sfx).c_str(), p.whole(true), true, p);
    }
    {  // a re-binning must join the extra streams first
      Proto p;
      bool ok = p.rebin() && p.launch(S, true) && p.launch(S, false, true);
      Proto q = p;
      expect(("rebin_without_join_reported" + sfx).c_str(), q.rebin(false), false, q);
      expect(("rebin_after_join" + sfx).c_str(), ok && p.rebin(true), true, p);
    }
  }
  {  // host synchronisation orders everything before it
    Proto p;
    bool ok = p.rebin() && p.launch(2, true) && p.launch(2, false);
    for (int s = 0; s < kHzStreams; ++s) p.h.sync(s);
    p.pending = 0;
    expect("whole_launch_after_host_sync", ok && p.whole(false), true, p);
  }
  {  // Binning: the host's picture of the device's binning (nx = 64: 16 tiles of 16 cells, 512 lanes)
    const int64_t nx = 64;
    const double dx = 0.1;
    Binning b;
    b.rebinned(16, 16, 512, true);
    expect("binning_source_gather_pending_not_tiled", b.tiled_for(4), false);
    b.tile_launched(true, nx, dx);
    expect("binning_tiled_after_launch", b.tiled_for(4) && !b.tiled_for(3), true);
    expect("binning_keys_valid_after_counting_launch", b.keys_valid_for(16, nx, dx), true);
    expect("binning_keys_other_grid_or_bins",
           b.keys_valid_for(16, 2 * nx, dx) || b.keys_valid_for(16, nx, 2 * dx) || b.keys_valid_for(9, nx, dx), false);
    for (int how = 0; how < 4; ++how) {  // each of these makes the keys stale
      Binning k = b;
      if (how == 0) k.per_packet_launched();
      if (how == 1) k.packets_replaced();
      if (how == 2) k.invalidate();
      if (how == 3) k.tile_launched(false, nx, dx);
      expect(("binning_keys_stale_" + std::to_string(how)).c_str(), k.keys_valid_for(16, nx, dx), false);
    }
    // the count-memset guard: counts 4..15 still hold the 16-bin counting launch
    b.invalidate();
    b.rebinned(4, 32, 512, false);
    expect("binning_memset_guard_larger_count", b.needs_count_memset(9) && !b.needs_count_memset(4), true);
    b.rebinned(9, 22, 512, false);
    expect("binning_memset_guard_after_rebin", !b.needs_count_memset(9) && b.needs_count_memset(16), true);
    b.invalidate();  // (the device's counts are as the scan left them: the skip stays legitimate)
    expect("binning_memset_skip_survives_invalidate", b.needs_count_memset(9), false);
    // invalidate(): the queries about the binning answer as for a new context
    b.rebinned(16, 16, 512, false);
    b.tile_launched(true, nx, dx);
    b.stepped(3);
    b.ode23_sorted();
    b.ode23_order_built();
    b.invalidate();
    const Binning fresh;
    bool same = b.tiled_for(4) == fresh.tiled_for(4) && b.keys_valid_for(16, nx, dx) == fresh.keys_valid_for(16, nx, dx);
    same = same && b.due(4) == fresh.due(4) && b.steps_left(4) == fresh.steps_left(4);
    same = same && b.src_pending() == fresh.src_pending() && b.ode23_order() == fresh.ode23_order();
    same = same && b.ode23_is_sorted() == fresh.ode23_is_sorted() && !b.tiled_for(4) && b.due(4);
    expect("binning_invalidate_as_constructed", same, true);
    // the re-binning cadence
    b.rebinned(16, 16, 512, true);
    b.stepped(3);
    expect("binning_cadence", !b.due(4) && b.steps_left(4) == 1, true);
    b.stepped(1);
    expect("binning_due_after_cycle", b.due(4), true);
  }
  {  // SetRing: the two rotations
    SetRing<int> r{0, 1, 2};
    r.flip();
    bool ok = r.cur == 1 && r.out == 0 && r.park == 2;
    r.park_cur();
    ok = ok && r.cur == 0 && r.out == 2 && r.park == 1;
    expect("set_ring_rotations", ok, true);
  }
  {  // SeriesExtent: frames of 8 words, a minimum of 4096 frames
    const int64_t per = 8, minimum = 4096;
    SeriesExtent e;
    expect("series_empty_does_not_fit", e.fits(1, per), false);
    expect("series_growth_from_empty_takes_minimum", e.grown(1, per, minimum) == minimum, true);
    e.reserved(minimum, per);
    expect("series_fits_up_to_capacity", e.fits(minimum, per) && !e.fits(minimum + 1, per), true);
    e.committed(minimum);
    expect("series_growth_doubles", !e.fits(1, per) && e.grown(1, per, minimum) == 2 * minimum, true);
    expect("series_growth_takes_needed", e.grown(3 * minimum, per, minimum) == 4 * minimum, true);
    SeriesExtent none;  // (no capacity at all, nor a minimum: the history)
    expect("series_extra_zero_never_grows", e.fits(0, per) && none.fits(0, per) && none.fits(0, 0), true);
    expect("series_no_minimum_takes_needed", none.grown(3, per, 0) == 3, true);
    expect("series_range_inside", e.holds(0, minimum) && e.holds(minimum, 0) && e.holds(minimum - 1, 1), true);
    expect("series_range_past_end", e.holds(0, minimum + 1) || e.holds(minimum, 1) || e.holds(minimum + 1, 0), false);
    expect("series_range_negative", e.holds(-1, 1) || e.holds(0, -1) || e.holds(-1, 0), false);
    e.cleared();
    expect("series_cleared_keeps_capacity", e.frames() == 0 && e.capacity(per) == minimum && e.fits(minimum, per), true);
    expect("series_cleared_holds_nothing", e.holds(0, 0) && !e.holds(0, 1), true);
    e.released();
    expect("series_released_drops_capacity", e.frames() == 0 && e.capacity(per) == 0 && !e.fits(1, per), true);
    // the history rule: 10 frames reserved for 512 packets (2 x 512 words a
    // frame) do not admit 10 frames of 4096 packets, only the one that fits
    SeriesExtent h;
    h.reserved(10, 2 * 512);
    expect("series_history_smaller_frame_does_not_pass",
           h.fits(10, 2 * 512) && !h.fits(10, 2 * 4096) && h.fits(1, 2 * 4096) && !h.fits(2, 2 * 4096), true);
    expect("series_history_growth_for_larger_frame", h.grown(10, 2 * 4096, 0) == 10, true);
  }
  {  // PlaneLayout at nw = 5, n2 = 3 against the four series' own formulas, worked out by hand:
     // a 5 x 7 plane; tails nq + 4, 3 (ns + 2) + 3, 3 (nw + 2) + (na + 2) + 2, 3 (nw + 2) + 2 (no + 2) + 2
    const PlaneLayout cond{5, 3, 0, 1, 2}, trans{5, 3, 0, 3, 3}, refr{5, 3, 3, 1, 2}, absfreq{5, 3, 3, 2, 2};
    expect("plane_layout_cond", cond.frame() == 35 && cond.nsums() == 5 && cond.tail() == 7, true);
    expect("plane_layout_trans", trans.frame() == 35 && trans.nsums() == 15 && trans.tail() == 18, true);
    expect("plane_layout_refr", refr.frame() == 35 && refr.nsums() == 26 && refr.tail() == 28, true);
    expect("plane_layout_absfreq", absfreq.frame() == 35 && absfreq.nsums() == 31 && absfreq.tail() == 33, true);
  }
  std::printf("%s\n", fails ? "FAILED" : "ALL OK");
  return fails ? 1 : 0;
}
