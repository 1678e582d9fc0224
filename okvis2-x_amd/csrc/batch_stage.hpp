// batch_stage.hpp — the staging layout of one call's arrays: a call-scoped batch (batch_calls.cpp)
// or what a batch-wide call on the resident batch takes up and brings down (okvisgpu_update_landmarks
// and okvisgpu_covisibilities, resident_calls.cpp): the library's one way to place arrays in
// batchScratch and the pinned stage. Every array the call's kernels read or write is declared once,
// with its element type (the device field's) and its element count, against the field of the
// device struct, or the local pointer, that will point to it. The layout is
// shared by a device buffer and a host staging buffer of the same shape, so that one copy takes
// every input up and one copy brings every output down:
//
//   [0, upEnd)            in | inout   uploaded
//   [downBegin, downEnd)  inout | out  read back
//   [downEnd, size)       scratch      device only (the host buffer need not cover it)
//
// Slots are ordered by kind, not by declaration, and each starts at a multiple of 256 bytes and
// takes at least 8, so an empty array still has an address of its own. An optional array that is
// absent is simply not declared: its field keeps the null it was initialised with.
//
// No HIP here: the two copies, the buffers and the synchronise belong to the context
// (okvisgpu_ctx::beginBatch / uploadBatch / finishBatch, runtime.hpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

namespace okg {

// A declared array whose staged host bytes the caller reads or writes (BatchLayout::host).
template <class T>
struct BatchSlot {
  int index;
};

class BatchLayout {
  template <class P>
  using Elem = std::remove_const_t<std::remove_pointer_t<P>>;

 public:
  // Uploaded from src; a null src reserves the slot for the caller to fill through host().
  template <class P>
  BatchSlot<Elem<P>> in(P& field, const void* src, size_t count) {
    return add(kIn, field, src, nullptr, count);
  }
  // Uploaded from src and read back; delivered to dst unless it is null.
  template <class P>
  BatchSlot<Elem<P>> inout(P& field, const void* src, void* dst, size_t count) {
    return add(kInout, field, src, dst, count);
  }
  // Read back; delivered to dst unless it is null (the slot is then read through host()).
  template <class P>
  BatchSlot<Elem<P>> out(P& field, void* dst, size_t count) {
    return add(kOut, field, nullptr, dst, count);
  }
  template <class P>
  void scratch(P& field, size_t count) {
    add(kScratch, field, nullptr, nullptr, count);
  }

  // Assigns the offsets; nothing is declared after it.
  void commit() {
    size_t size = 0;
    bool anyDown = false;
    for (int kind = kIn; kind <= kScratch; ++kind) {
      for (Slot& s : slots_) {
        if (s.kind != kind) continue;
        s.off = (size + 255) & ~size_t(255);
        size = s.off + std::max<size_t>(s.bytes, 8);
        if ((kind == kInout || kind == kOut) && !anyDown) {
          downBegin_ = s.off;
          anyDown = true;
        }
      }
      if (kind == kInout) upEnd_ = size;
      if (kind == kOut) downEnd_ = size;
    }
    if (!anyDown) downBegin_ = downEnd_;
    size_ = size;
  }
  size_t upEnd() const { return upEnd_; }
  size_t downBegin() const { return downBegin_; }
  size_t downEnd() const { return downEnd_; }  // >= upEnd(): what the host buffer holds
  size_t size() const { return size_; }        // what the device buffer holds

  // Binds a host buffer of downEnd() bytes and a device buffer of size() bytes: every declared
  // field points into the device buffer, every source is copied into the host buffer.
  void begin(char* host, char* dev) {
    host_ = host;
    dev_ = dev;
    for (const Slot& s : slots_) {
      s.patch(s.field, dev + s.off);
      if (s.src && s.bytes) std::memcpy(host + s.off, s.src, s.bytes);
    }
  }
  char* hostBase() const { return host_; }
  char* devBase() const { return dev_; }
  template <class T>
  T* host(BatchSlot<T> s) const {
    return reinterpret_cast<T*>(host_ + slots_[(size_t)s.index].off);
  }
  // After [downBegin, downEnd) came back into the host buffer: every output to its destination.
  void deliver() const {
    for (const Slot& s : slots_)
      if (s.dst && s.bytes) std::memcpy(s.dst, host_ + s.off, s.bytes);
  }

 private:
  enum Kind { kIn, kInout, kOut, kScratch };
  struct Slot {
    int kind;
    void* field;
    void (*patch)(void* field, char* p);
    const void* src;
    void* dst;
    size_t bytes, off;
  };
  template <class P>
  BatchSlot<Elem<P>> add(int kind, P& field, const void* src, void* dst, size_t count) {
    static_assert(std::is_pointer<P>::value && !std::is_void<Elem<P>>::value, "a typed pointer field");
    slots_.push_back({kind, &field, [](void* f, char* p) { *static_cast<P*>(f) = reinterpret_cast<P>(p); }, src, dst,
                      sizeof(Elem<P>) * count, 0});
    return {(int)slots_.size() - 1};
  }
  std::vector<Slot> slots_;
  size_t upEnd_ = 0, downBegin_ = 0, downEnd_ = 0, size_ = 0;
  char *host_ = nullptr, *dev_ = nullptr;
};

}  // namespace okg
