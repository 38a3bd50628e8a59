// qa_stage.h — how the host forms of the queries stage through qa_ctx::stageQuery: the only code that computes an offset into it.
// A host form declares its planes, one line each, in the order its copies are to run: the declarations are the layout.  The layout
// half includes no HIP header (tests/cpp/stage_check.cpp compiles it alone under a host compiler); QueryStage is hipcc's only.
// A plane the caller did not ask for takes no room and resolves to nullptr, which every shared body takes as "not wanted", as it
// does from the device forms.  There is no always-present plane: no body needs one that the caller left out.
#pragma once
#include <cassert>
#include <cstddef>

// Planes appended as (element size, count, wanted): each starts on a multiple of 16 bytes, one that is not wanted has no bytes,
// and the running total is what to reserve.  size_t throughout: 2^31 - 1 probes of 1.2 MB each do not wrap
struct StageLayout {
  static const int kMaxPlanes = 16;
  size_t off[kMaxPlanes], bytes[kMaxPlanes], total = 0;
  int count = 0;
  int Add(size_t elemSize, size_t n, bool wanted)
  {
    assert(count < kMaxPlanes);
    off[count] = total;
    bytes[count] = wanted ? elemSize * n : 0;
    total += (bytes[count] + 15) & ~(size_t) 15;
    return count++;
  }
  void *At(void *base, int i) const { return bytes[i] ? static_cast<unsigned char *>(base) + off[i] : nullptr; }
};

#ifdef __HIPCC__
#include "qa_ctx.h"

// In(host, count) is copied to the device by Begin() and Out(host, count) back by End(), each when host is given.  Begin() reserves,
// End() synchronises; the copies run in declaration order on c->stream.  Between the two, st(plane) is the plane's device pointer
// (none is known before the reservation, hence the handle).  A body that refuses after Begin() returns without End(), as before
class QueryStage {
 public:
  template <class T> struct Plane { int i; };
  explicit QueryStage(qa_ctx *c) : c_(c) {}
  template <class T> Plane<T> In(const T *host, size_t n) { const int i = lay_.Add(sizeof(T), n, host != nullptr); in_[i] = host; return {i}; }
  template <class T> Plane<T> Out(T *host, size_t n) { const int i = lay_.Add(sizeof(T), n, host != nullptr); out_[i] = host; return {i}; }
  template <class T> T *operator()(Plane<T> p) const { return static_cast<T *>(lay_.At(c_->stageQuery.p, p.i)); }
  int Begin()
  {
    HIP_TRY(c_->stageQuery.Reserve(lay_.total));
    for (int i = 0; i < lay_.count; ++i)
      if (in_[i] && lay_.bytes[i]) HIP_TRY(hipMemcpyAsync(lay_.At(c_->stageQuery.p, i), in_[i], lay_.bytes[i], hipMemcpyHostToDevice, c_->stream));
    return QA_OK;
  }
  int End()
  {
    for (int i = 0; i < lay_.count; ++i)
      if (out_[i] && lay_.bytes[i]) HIP_TRY(hipMemcpyAsync(out_[i], lay_.At(c_->stageQuery.p, i), lay_.bytes[i], hipMemcpyDeviceToHost, c_->stream));
    HIP_TRY(hipStreamSynchronize(c_->stream));
    return QA_OK;
  }

 private:
  qa_ctx *c_;
  StageLayout lay_;
  const void *in_[StageLayout::kMaxPlanes] = {};   // the host side of each plane: at most one of the two is set
  void *out_[StageLayout::kMaxPlanes] = {};
};
#endif
