// swrt_packet_state.hpp — the host's bookkeeping of the packet steppers: which
// of the three packet sets is which (SetRing), the host's picture of the
// device's binning (Binning), the frame series' counting (SeriesExtent) and
// the class-plane series' frame layout (PlaneLayout).  Plain host code, no HIP type: the library uses
// it in swrt_ctx, the CPU model tests/hazard_model.cpp on its own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace swrt {

// Three packet sets of handle type S: the packets, the next launch's output
// and a parked third set, traded by two named rotations.
template <typename S>
struct SetRing {
  S cur, out, park;
  // (cur, out) <- (out, cur): the launch's output becomes the packets
  void flip() { std::swap(cur, out); }
  // (cur, out, park) <- (out, park, cur): the old packets, which a split
  // source-gather launch may still read, are parked until the next re-binning
  void park_cur() { std::swap(cur, out), std::swap(out, park); }
};

// What the host knows of the binning the device holds (keys, counts, tile
// starts and order, the packets' order).  Only the transitions change it.
class Binning {
 public:
  // The binning is stale (new packets or launch settings, a corrupted count):
  // the next packet call re-bins before it reads anything else here.  The
  // device's count block is untouched, so counts_zero_ stays.
  void invalidate() {
    valid_ = keys_fresh_ = src_pending_ = o23_order_ = o23_sorted_ = false;
    steps_ = 0;
  }
  // A re-binning into `nbins` bins of `tile` cells a side was queued, its tile
  // order ranked for `lanes`-wide workgroups.  indirect: the packets were not
  // moved, the next tile launch reads them through the source index.
  void rebinned(int nbins, int tile, int lanes, bool indirect) {
    invalidate();
    valid_ = counts_zero_ = true;  // (the scan cleared the counts it read)
    nbins_ = nbins, tile_ = tile, lanes_ = lanes;
    src_pending_ = indirect;
    cells_sorted_ = false;
  }
  // A tile launch wrote the packets in cell order.  counted_next: it also wrote
  // the next binning's keys and counts, for a grid of nx cells of size dx (the
  // keys depend on those only, not on the field values).
  void tile_launched(bool counted_next, int64_t nx, double dx) {
    src_pending_ = false;
    cells_sorted_ = true;
    keys_fresh_ = counted_next;
    if (counted_next) counts_zero_ = false, key_nx_ = nx, key_dx_ = dx;
  }
  void per_packet_launched() { keys_fresh_ = false; }               // the packets moved in place
  void packets_replaced() { keys_fresh_ = cells_sorted_ = false; }  // other buffers became the packets
  void stepped(int64_t n) { steps_ += n; }                          // leapfrog steps since the re-binning
  void ode23_order_built() { o23_order_ = true; }  // the ode23 order array holds this binning's in-tile cell order
  void ode23_sorted() { o23_sorted_ = true, o23_since_ = 0; }  // the packets themselves are in that order
  bool ode23_call_due(int every) { return ++o23_since_ >= every; }  // one more ode23 call; true: re-bin first

  // a binning into ntx x ntx tiles is in force and the packets are in its order
  bool tiled_for(int ntx) const { return valid_ && !src_pending_ && nbins_ == ntx * ntx; }
  // the last tile launch left the keys and counts of exactly this binning
  bool keys_valid_for(int nbins, int64_t nx, double dx) const {
    return keys_fresh_ && valid_ && nbins == nbins_ && key_nx_ == nx && key_dx_ == dx;
  }
  // No memset when the last scan zeroed exactly these counts (the same bin
  // count, no counting launch since).  Counts past the last scan's bins may
  // hold an older, larger binning's counting launch, hence the equal count.
  bool needs_count_memset(int nbins) const { return !(counts_zero_ && nbins_ == nbins); }
  bool due(int64_t every) const { return !valid_ || steps_ >= every; }
  int64_t steps_left(int64_t every) const { return every - steps_; }
  int nbins() const { return nbins_; }
  int tile() const { return tile_; }
  int lanes() const { return lanes_; }  // the workgroup width the tile order was ranked for
  bool counts_zero() const { return counts_zero_; }
  bool src_pending() const { return src_pending_; }
  bool cells_sorted() const { return cells_sorted_; }  // packets of every tile are in cell order
  bool ode23_order() const { return o23_order_; }
  bool ode23_is_sorted() const { return o23_sorted_; }

 private:
  bool valid_ = false, keys_fresh_ = false, counts_zero_ = false, src_pending_ = false, cells_sorted_ = false;
  bool o23_order_ = false, o23_sorted_ = false;
  int nbins_ = 0, tile_ = 0, lanes_ = 0, o23_since_ = 0;
  int64_t steps_ = 0, key_nx_ = 0;
  double key_dx_ = 0.0;
};

// How far a series of fixed-size frames in a growable buffer has got: the
// frames recorded and the capacity allocated.  The capacity is kept in words,
// not frames, and asked for in frames of the caller's current size `per`: the
// history's frame is 2 x n words and n changes with every swrt_packets_set, so
// a frame count reserved for a smaller frame must not pass the check.
class SeriesExtent {
 public:
  int64_t frames() const { return frames_; }
  int64_t capacity(int64_t per) const { return per > 0 ? words_ / per : 0; }  // in frames of `per` words
  // `extra` more frames of `per` words fit (nothing more always does)
  bool fits(int64_t extra, int64_t per) const { return extra <= 0 || frames_ + extra <= capacity(per); }
  // the capacity, in frames, to grow to when they do not: at least `minimum`
  int64_t grown(int64_t extra, int64_t per, int64_t minimum) const {
    return std::max<int64_t>({minimum, 2 * capacity(per), frames_ + extra});
  }
  // [first, first + count) lies inside the recorded frames
  bool holds(int64_t first, int64_t count) const { return !(first < 0 || count < 0 || first + count > frames_); }

  void reserved(int64_t cap, int64_t per) { words_ = cap * per; }  // buffers for `cap` frames of `per` words are in place
  void committed(int64_t count) { frames_ += count; }              // `count` more frames were queued
  void cleared() { frames_ = 0; }                                  // the series starts again in the same buffers
  void released() { frames_ = words_ = 0; }                        // the buffers are gone

 private:
  int64_t frames_ = 0, words_ = 0;
};

// A class-plane frame (the conditional, transition, refraction and
// absolute-frequency series): a count plane over the omega classes and the
// classes of a second axis, under- and overflow included, then a tail of
// per-class sums followed by a few stats words.
struct PlaneLayout {
  int nw = 0, n2 = 0;                       // omega classes, classes of the second axis
  int wsums = 0, csums = 0, stats = 0;      // sums per omega class, per second-axis class; stats words
  size_t frame() const { return (size_t)(n2 + 2) * (nw + 2); }
  size_t nsums() const { return (size_t)wsums * (nw + 2) + (size_t)csums * (n2 + 2); }
  size_t tail() const { return nsums() + stats; }
};

}  // namespace swrt
