// The scratch arena of the synchronous "upload, launch, read back" entries (audit_host.hip, forecast_host.hip, road_host.hip): a field is
// declared ONCE, with its element type and count; the handle that comes back knows its offset and its bytes, hands out the typed pointer
// under any base (the device scratch for a launch, a host image for an upload) and feeds the upload and the read-back.  No HIP call, no
// context: tests compile this header alone.
#pragma once
#include <cstddef>

// every field starts on a 16-byte boundary: k_road_boxes reads `verts` as double2, one 16-byte load per vertex
constexpr size_t AR_ALIGN = 16;

template <class T>
struct ArField {
  size_t off = 0, n = 0;                            // byte offset in the arena, elements
  size_t bytes() const { return n * sizeof(T); }
  size_t end() const { return off + bytes(); }
  T *at(char *base) const { return reinterpret_cast<T *>(base + off); }
};

struct Arena {
  size_t top = 0;                                   // bytes taken so far = the end of the last field
  template <class T>
  ArField<T> take(size_t n) {                       // (a field of no element takes no byte; the next one aligns itself)
    ArField<T> f;
    f.off = (top + AR_ALIGN - 1) & ~(AR_ALIGN - 1);
    f.n = n;
    top = f.end();
    return f;
  }
};

// a field on its way back to the host: the host pointer must be a pointer to the field's own element type
struct ArBack {
  void *h;
  size_t off, bytes;
  template <class T>
  ArBack(T *host, const ArField<T> &f) : h(host), off(f.off), bytes(f.bytes()) {}
};
