// pba_alloc.h -- THE bookkeeping of a handle's device and pinned memory: a registry of allocations keyed by the address of the pointer
// field that owns each one.  A buffer is entered in one place (its reserve call); nothing else lists it, and release_all frees whatever
// was reserved.  The registry reaches the runtime only through MemBackend, so no HIP header is needed: plain C++ compiles it
// (tests/native/alloc_probe.cpp runs it over malloc); pba_handle.h holds the HIP backend.
#pragma once
#include <stddef.h>

#include <unordered_map>

namespace pba {

// mapped: pinned host memory the device reads and writes in place; a second field holds its device address
enum class MemKind { device, pinned, mapped };

// What the registry needs of a runtime.  alloc / device_view return 0, or the runtime's error code.
struct MemBackend {
  virtual int alloc(MemKind kind, size_t bytes, void** out) = 0;
  virtual void free(MemKind kind, void* p) = 0;
  virtual int device_view(void* host, void** out) = 0;
};

class Allocations {
 public:
  explicit Allocations(MemBackend* backend) : backend_(backend) {}
  Allocations(const Allocations&) = delete;
  Allocations& operator=(const Allocations&) = delete;

  // Grow-only: room for n elements (n == 0 counts as 1) behind *field.  A buffer that is large enough is kept; otherwise the old one is
  // freed and bytes + bytes / 8 allocated (a little headroom against frame-to-frame jitter), so the contents are undefined after the
  // call (every user overwrites or uploads the whole buffer).
  // kind mapped: *view receives the block's device address.  Returns 0, or the backend's error code: then *field (and *view) are null
  // and the registry holds no entry for the field.
  template <class T>
  int reserve(T** field, MemKind kind, size_t n, T** view = nullptr) {
    return reserve_bytes(reinterpret_cast<void**>(field), kind, (n ? n : 1) * sizeof(T), reinterpret_cast<void**>(view));
  }
  template <class T>
  void release(T** field) {
    auto it = entries_.find(reinterpret_cast<void**>(field));
    if (it == entries_.end()) return;
    free_entry(it->first, it->second);
    entries_.erase(it);
  }
  // Exchanges the buffers behind two fields of the same kind (a buffer filled on the side takes the place of the one it was filled
  // from); each field keeps the other's size.  Both must have been reserved.
  template <class T>
  void exchange(T** a, T** b) {
    auto ia = entries_.find(reinterpret_cast<void**>(a)), ib = entries_.find(reinterpret_cast<void**>(b));
    if (ia == entries_.end() || ib == entries_.end() || ia->second.kind != ib->second.kind) return;
    T* t = *a; *a = *b; *b = t;
    const size_t n = ia->second.bytes; ia->second.bytes = ib->second.bytes; ib->second.bytes = n;
  }
  void release_all() {
    for (auto& kv : entries_) free_entry(kv.first, kv.second);
    entries_.clear();
  }
  // Forgets everything and frees nothing (the fields keep their values): for a handle whose device still holds work that may touch the
  // buffers and will never finish.
  void abandon() { entries_.clear(); }

  size_t count() const { return entries_.size(); }

 private:
  struct Entry {
    MemKind kind;
    size_t bytes;
    void** view;   // mapped only
  };

  void free_entry(void** field, const Entry& en) {
    backend_->free(en.kind, *field);
    *field = nullptr;
    if (en.view) *en.view = nullptr;
  }
  int reserve_bytes(void** field, MemKind kind, size_t bytes, void** view) {
    auto it = entries_.find(field);
    if (it != entries_.end()) {
      if (it->second.bytes >= bytes) return 0;
      free_entry(field, it->second);
      entries_.erase(it);
    }
    const size_t want = bytes + bytes / 8;
    void* p = nullptr;
    int rc = backend_->alloc(kind, want, &p);
    if (rc) return rc;
    if (kind == MemKind::mapped && (rc = backend_->device_view(p, view))) {
      backend_->free(kind, p);
      *view = nullptr;
      return rc;
    }
    *field = p;
    entries_[field] = Entry{kind, want, kind == MemKind::mapped ? view : nullptr};
    return 0;
  }

  MemBackend* backend_;
  std::unordered_map<void**, Entry> entries_;
};

}  // namespace pba
