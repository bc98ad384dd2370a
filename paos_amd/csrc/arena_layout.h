// arena_layout.h -- where the blocks of the parameter arena go: the rounding of a block, whether a run of blocks fits the
// slab being filled, and the range that has been written to the pinned slab but not copied to the device yet.  Pure
// offset arithmetic in doubles: no HIP, no context, so that a plain C++ program can test it (tests/arena_layout_main.cpp).
// context.hip wraps it with the pinned and device memory and the copies (ArenaBatch, host.h).
#pragma once
#include <cstddef>

#pragma GCC visibility push(hidden)  // internal to the library, like everything host.h declares

// every block starts at a multiple of 16 doubles (128 B) of its slab
constexpr size_t kArenaAlign = 16;
inline size_t arena_rounded(size_t count) { return (count + kArenaAlign - 1) & ~(kArenaAlign - 1); }
// added to every reservation: callers that sum unrounded sizes are covered for the rounding of a few blocks
constexpr size_t kArenaSlack = 64;

enum ArenaRoom {
  ARENA_FITS,    // behind the head of the slab being filled
  ARENA_SWITCH,  // in an empty slab: go to the next one first
  ARENA_GROW     // in no slab: every slab has to grow first
};

// The fill of the slab being filled.  [0, sent): copied to the device (or on its way); [sent, head): written to the pinned
// slab only -- the pending range, which the next commit copies in one transfer.  head and sent are multiples of kArenaAlign.
struct ArenaLayout {
  size_t cap = 0;   // doubles per slab, a multiple of kArenaAlign
  size_t head = 0;  // where the next block goes
  size_t sent = 0;  // everything below has been handed to a copy

  // room for `total` doubles (plus kArenaSlack) that must stay in ONE slab
  ArenaRoom room(size_t total) const {
    total += kArenaSlack;
    if (total > cap) return ARENA_GROW;
    return head + total > cap ? ARENA_SWITCH : ARENA_FITS;
  }
  // the capacity that holds `total` (plus kArenaSlack): doubled until it does
  size_t grown(size_t total) const {
    size_t c = cap ? cap : kArenaAlign;
    while (c < total + kArenaSlack) c *= 2;
    return c;
  }
  // does one block of `count` doubles fit behind the head?  (a block may end at the slab's end; its rounding may not pass it)
  bool fits(size_t count) const { return count <= cap && head + count <= cap; }
  // place a block that fits(): its offset; the head moves on by the rounded size (cap and head are multiples of
  // kArenaAlign, so the rounding of a block that fits ends at the slab's end at the latest)
  size_t place(size_t count) {
    const size_t at = head;
    head += arena_rounded(count);
    return at;
  }
  bool pending() const { return sent < head; }
  // hand the pending range over to a copy: [*first, *first + *count); false if nothing is pending
  bool take(size_t* first, size_t* count) {
    if (!pending()) return false;
    *first = sent;
    *count = head - sent;
    sent = head;
    return true;
  }
  void drop() { sent = head; }               // an error path: the pending range is never copied (the head stays advanced)
  void rewind() { head = sent = 0; }         // a fresh slab
};

// One batch of blocks: begin (optional) .. add .. add .. commit.  A batch that was begun holds its reservation: a block
// that does not fit is an error, never a switch of slabs (its earlier blocks would stay behind).  After commit the batch
// is closed: a later add is refused, since the launches behind the commit may already be reading.
struct ArenaBatchState {
  bool reserved = false, closed = false;
  bool may_add() const { return !closed; }
  bool may_switch() const { return !reserved; }
};

#pragma GCC visibility pop
