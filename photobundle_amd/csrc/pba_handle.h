// pba_handle.h -- the plumbing the three handles (pba_engine, pba_stereo, pba_sgm) share: the HIP backend of the allocation registry
// (pba_alloc.h), a base with the handle's device, stream, error text, registry and events, one fail / PBA_HIP_TRY, the texts of failed
// create calls, and a scope guard for a call's temporary device buffer.  The runtime's allocation, free and event calls of the
// handles are written in this file only: what it releases is everything a handle holds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/pba.h"
#include "pba_alloc.h"

namespace pba {

struct HipBackend final : MemBackend {
  int alloc(MemKind kind, size_t bytes, void** out) override {      // (the registry hands the codes back: hipError_t)
    if (kind == MemKind::device) return (int)hipMalloc(out, bytes);
    return (int)hipHostMalloc(out, bytes, kind == MemKind::mapped ? hipHostMallocMapped : hipHostMallocDefault);
  }
  void free(MemKind kind, void* p) override {
    if (kind == MemKind::device) (void)hipFree(p);
    else (void)hipHostFree(p);
  }
  int device_view(void* host, void** out) override { return (int)hipHostGetDevicePointer(out, host, 0); }
};
inline HipBackend g_hip_backend;   // stateless

struct Handle {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  Allocations mem{&g_hip_backend};
  std::vector<hipEvent_t*> events;   // the event fields handle_event filled
};

inline int fail(Handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  return code;
}

#define PBA_HIP_TRY(h, call)                                                                           \
  do {                                                                                                 \
    hipError_t _r = (call);                                                                            \
    if (_r != hipSuccess) return pba::fail((h), PBA_ERR_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
  } while (0)

// Is there a device of that index?  (a create call asks before it builds anything)
inline bool device_exists(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) == hipSuccess && device >= 0 && device < n) return true;
  (void)hipGetLastError();
  return false;
}
// Selects the device and creates the handle's stream.
inline int handle_open(Handle* h, int device) {
  h->device = device;
  PBA_HIP_TRY(h, hipSetDevice(device));
  PBA_HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  return PBA_OK;
}
inline int handle_event(Handle* h, hipEvent_t* ev, unsigned flags = hipEventDefault) {
  PBA_HIP_TRY(h, hipEventCreateWithFlags(ev, flags));
  h->events.push_back(ev);
  return PBA_OK;
}
// The end of a handle, in the order every destroy keeps: the caller selects the device and waits for the stream (handle_drain), shuts
// down what else uses the memory, then memory, events and stream go (handle_close).
inline void handle_drain(Handle* h) {
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
}
inline void handle_close(Handle* h) {
  h->mem.release_all();
  for (hipEvent_t* ev : h->events) { (void)hipEventDestroy(*ev); *ev = nullptr; }
  h->events.clear();
  if (h->stream) { (void)hipStreamDestroy(h->stream); h->stream = nullptr; }
}
// ... and a handle with nothing in between
template <class H>
void handle_destroy(H* h) {
  if (!h) return;
  handle_drain(h);
  handle_close(h);
  delete h;
}

// A create call that fails has no handle to keep its message: <type>_last_error(NULL) reads it from a thread-local text, one per
// handle type H (pba_stereo_last_error(NULL) never shows an SGM message).
template <class H>
std::string& create_error() {
  thread_local std::string text;
  return text;
}
template <class H>
int create_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  create_error<H>() = buf;
  return code;
}
// ... and one that fails with a half-built handle: its message is kept, the handle destroyed
template <class H>
int create_bail(H* h, int code, void (*destroy)(H*)) {
  create_error<H>() = h->err;
  destroy(h);
  return code;
}

// A call's temporary device buffer: freed when the scope ends, on every path.
template <class T>
struct DeviceTemp {
  T* p = nullptr;
  DeviceTemp() = default;
  DeviceTemp(const DeviceTemp&) = delete;
  DeviceTemp& operator=(const DeviceTemp&) = delete;
  ~DeviceTemp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)); }
};

}  // namespace pba
