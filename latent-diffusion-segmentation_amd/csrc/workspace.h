// The per-forward activation workspace of a handle: one device allocation, a persist region (bump) in front and a scratch
// region (stack) behind it.  Pure host C++ with no HIP include, like the *_plan.h headers: tests/test_workspace_cpu.py
// replays it on the host alone.
//
// Every pass runs twice (runtime.h, plan_workspace / plan_and_run): dry, which only measures the two peaks, and real, on an
// allocation of rup(persist_peak, 4096) + rup(scratch_peak, 4096) bytes with the scratch region starting at the first term.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>

namespace ldmseg::rt {

inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Workspace {  // per-forward activations: persist (bump) + scratch (stack)
  char* base = nullptr;
  size_t cap = 0;
  size_t persist_top = 0, scratch_top = 0, scratch_base = 0;
  size_t persist_peak = 0, scratch_peak = 0;
  bool dry = false;
  bool overflow = false;   // a non-dry request went past the planned capacity (stale plan): the forward fails instead of writing out of range
  void begin(bool dry_, size_t scratch_base_) {
    dry = dry_;
    overflow = false;
    persist_top = 0;
    scratch_base = scratch_base_;
    scratch_top = 0;
    persist_peak = scratch_peak = 0;
  }
  void* persist(size_t bytes) {
    const size_t off = persist_top;
    persist_top += rup(bytes, 256);
    if (persist_top > persist_peak) persist_peak = persist_top;
    if (!dry && persist_top > (scratch_base ? scratch_base : cap)) { overflow = true; return base; }
    return dry ? (void*)(uintptr_t)(0x1000 + off) : base + off;
  }
  void* scratch(size_t bytes) {
    const size_t off = scratch_top;
    scratch_top += rup(bytes, 256);
    if (scratch_top > scratch_peak) scratch_peak = scratch_top;
    if (!dry && scratch_base + scratch_top > cap) { overflow = true; return base; }
    return dry ? (void*)(uintptr_t)(0x1000 + off) : base + scratch_base + off;
  }
  size_t mark() const { return scratch_top; }
  void reset(size_t m) { scratch_top = m; }
};

// up to four shape numbers a pass's dry run depends on besides the handle itself (plan_workspace)
using PlanKey = std::array<int, 4>;

}  // namespace ldmseg::rt
