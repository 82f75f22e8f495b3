// Layout of one scratch buffer.  The same sequence of take() calls sizes it
// (base == nullptr) and places it (base == the buffer), so the two cannot
// drift apart.  Every array starts on a 256-byte boundary unless the caller
// asks for less (base is 256-byte aligned: hipMalloc's buffers are), so an
// array of odd length never misaligns the 8-byte atomics of the one behind it.
// A zero-length array takes no space and returns the current aligned position.
// Arrays that travel in one copy or one memset are taken as one block and
// split by the caller.  Host only, nothing from HIP: a plain C++ program can
// include this file (tests/test_carve.py).
#pragma once
#include <cstddef>
#include <cstdint>

struct Carve {
  uint8_t* base = nullptr;
  size_t used = 0;
  uint8_t* take_bytes(size_t bytes, size_t align = 256) {
    const size_t at = (used + align - 1) / align * align;
    if (bytes) used = at + bytes;
    return reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(base) + at);
  }
  template <class T>
  T* take(size_t count, size_t align = 256) {
    return reinterpret_cast<T*>(take_bytes(count * sizeof(T), align));
  }
};
