// Caller-owned workspaces (host only).  Every workspace has ONE layout function: it takes the shape parameters and a WsArena
// and fills the pointers of its argument record by take<T>(count), region after region.  Walked over a null base it is the size
// query (every pointer comes back null, bytes() is the answer); walked over the caller's pointer it is the carve.  Regions start
// on 256-byte boundaries; the base is aligned up, which bytes() pays for with 256.
#pragma once
#include <stdint.h>

static inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
static inline int64_t up256(int64_t v) { return align_up(v, 256); }

class WsArena {
 public:
  WsArena() : base_(nullptr), off_(0) {}                                   // sizing pass
  explicit WsArena(const void* workspace) : base_(reinterpret_cast<char*>(up256((int64_t)workspace))), off_(0) {}
  template <typename T>
  T* take(int64_t count) {
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += up256(count * (int64_t)sizeof(T));
    return p;
  }
  int64_t offset() const { return off_; }                                 // of the next region, from the aligned base
  char* base() const { return base_; }                                    // the aligned base (null in a sizing pass)
  int64_t bytes() const { return off_ + 256; }                            // what the caller must provide for the walk so far
  bool covers(int64_t workspace_bytes) const { return workspace_bytes >= bytes(); }

 private:
  char* base_;
  int64_t off_;
};

// the size query of a layout function `layout(shape..., WsArena&)`: its sizing pass
template <typename Layout, typename... Shape>
int64_t ws_bytes(Layout layout, Shape... shape) {
  WsArena ws;
  layout(shape..., ws);
  return ws.bytes();
}
