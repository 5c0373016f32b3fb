// The workspace allocator (csrc/workspace.h) on the host alone, the way a handle uses it: a seeded random sequence of persist /
// scratch / mark / reset calls is replayed dry (measuring the peaks) and then real, on a buffer sized and split as plan_workspace /
// plan_and_run do.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I latent-diffusion-segmentation_amd/csrc
//       tools/workspace_replay.cpp -o workspace_replay && ./workspace_replay [seed ...]
// Checked, per seed: (a) the real pass does not overflow and every range it hands out lies inside the buffer (the first and last
// byte of each are written, so the sanitizer sees a range that does not); (b) persist ranges end where the scratch region begins,
// and ranges that are live together are disjoint; (c) with room for one 256-byte unit less than either peak the pass reports
// overflow and the request that crossed gets `base`; (d) no dry pointer lies inside the real buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "workspace.h"

using namespace ldmseg::rt;

namespace {

enum Kind { PERSIST, SCRATCH, MARK, RESET };
struct Op { Kind kind; size_t arg; };      // bytes, or for RESET: how many marks to pop (0: reset(0), as the reconstruct chain does)

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

std::vector<Op> make_ops(uint64_t seed, int n) {
  Rng r{seed};
  std::vector<Op> ops;
  int depth = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t c = r.next() % 100;
    // sizes from one byte to a megabyte, not multiples of the 256-byte unit
    const size_t bytes = 1 + (r.next() % 4 == 0 ? r.next() % (1u << 20) : r.next() % (1u << 12));
    if (c < 15) ops.push_back({PERSIST, bytes});
    else if (c < 60) ops.push_back({SCRATCH, bytes});
    else if (c < 80) { ops.push_back({MARK, 0}); ++depth; }
    else if (depth > 0) { const size_t pop = c == 99 ? 0 : 1 + r.next() % depth; ops.push_back({RESET, pop}); depth = pop ? depth - (int)pop : 0; }
  }
  return ops;
}

struct Range { uintptr_t lo, hi; bool persist; };
struct Pass {
  std::vector<void*> ptrs;       // one per PERSIST / SCRATCH op
  std::vector<Range> ranges;
  int first_refused = -1;        // index into ptrs of the first request made after or at the overflow
  bool ok = true;
};

// replays `ops`; a real pass checks liveness-disjointness as it goes and touches both ends of every range
Pass replay(Workspace& ws, const std::vector<Op>& ops, bool touch) {
  Pass out;
  std::vector<size_t> marks;
  std::vector<std::pair<Range, size_t>> live;      // scratch ranges with the stack height they were made at
  uintptr_t persist_end = 0;
  for (const Op& op : ops) {
    if (op.kind == MARK) { marks.push_back(ws.mark()); continue; }
    if (op.kind == RESET) {
      size_t m = 0;
      if (op.arg == 0) marks.clear();
      else { for (size_t k = 0; k < op.arg; ++k) { m = marks.back(); marks.pop_back(); } }
      ws.reset(m);
      while (!live.empty() && live.back().second >= m) live.pop_back();
      continue;
    }
    const size_t top = ws.mark();
    void* p = op.kind == PERSIST ? ws.persist(op.arg) : ws.scratch(op.arg);
    out.ptrs.push_back(p);
    if (ws.overflow) {
      if (out.first_refused < 0) out.first_refused = (int)out.ptrs.size() - 1;
      continue;
    }
    const Range g{(uintptr_t)p, (uintptr_t)p + op.arg, op.kind == PERSIST};
    out.ranges.push_back(g);
    if (ws.dry) continue;
    if (g.persist) {
      if (g.lo < persist_end) { std::printf("persist ranges overlap\n"); out.ok = false; }
      persist_end = g.hi;
    } else {
      for (const auto& l : live)
        if (g.lo < l.first.hi && l.first.lo < g.hi) { std::printf("live scratch ranges overlap\n"); out.ok = false; }
      live.push_back({g, top});
    }
    if (touch) { ((volatile char*)p)[0] = 1; ((volatile char*)p)[op.arg - 1] = 1; }
  }
  return out;
}

bool check_seed(uint64_t seed, int n_ops) {
  const std::vector<Op> ops = make_ops(seed, n_ops);
  Workspace ws;
  ws.begin(true, 0);
  const Pass dry = replay(ws, ops, false);
  const size_t pp = ws.persist_peak, sp = ws.scratch_peak;
  if (pp <= 256 || sp <= 256) { std::printf("seed %llu: sequence too small\n", (unsigned long long)seed); return false; }
  const size_t sbase = rup(pp, 4096), cap = sbase + rup(sp, 4096);
  std::vector<char> buf(cap);
  ws.base = buf.data();
  ws.cap = cap;
  bool ok = true;
  auto expect = [&](bool c, const char* what) { if (!c) { std::printf("seed %llu: %s\n", (unsigned long long)seed, what); ok = false; } };

  ws.begin(false, sbase);
  const Pass real = replay(ws, ops, true);
  const uintptr_t lo = (uintptr_t)buf.data(), hi = lo + cap;
  expect(real.ok, "ranges live together overlap");
  expect(!ws.overflow && real.first_refused < 0, "(a) the real pass overflowed its own plan");
  expect(ws.persist_peak == pp && ws.scratch_peak == sp, "the real pass measured other peaks than the dry one");
  for (const Range& g : real.ranges) {
    expect(g.lo >= lo && g.hi <= hi, "(a) a range leaves the buffer");
    expect(g.persist ? g.hi <= lo + sbase : g.lo >= lo + sbase, "(b) a persist range meets the scratch region");
  }
  for (void* p : dry.ptrs) expect((uintptr_t)p < lo || (uintptr_t)p >= hi, "(d) a dry pointer lies inside the real buffer");

  // (c) one unit short of the persist peak (the scratch region starts one unit early), then of the scratch peak
  const size_t short_base[2] = {pp - 256, sbase}, short_cap[2] = {pp - 256 + rup(sp, 4096), sbase + sp - 256};
  for (int k = 0; k < 2; ++k) {
    ws.cap = short_cap[k];
    ws.begin(false, short_base[k]);
    const Pass p = replay(ws, ops, false);
    expect(ws.overflow && p.first_refused >= 0, "(c) a short workspace went unnoticed");
    if (p.first_refused >= 0) expect(p.ptrs[p.first_refused] == (void*)buf.data(), "(c) the refused request did not get base");
    for (const Range& g : p.ranges) expect(g.lo >= lo && g.hi <= lo + short_cap[k], "(c) a range before the overflow leaves the short buffer");
  }
  std::printf("seed %llu: %zu ops, persist peak %zu, scratch peak %zu: %s\n", (unsigned long long)seed, ops.size(), pp, sp, ok ? "ok" : "FAILED");
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  bool ok = true;
  if (argc < 2) ok = check_seed(1, 4000);
  for (int i = 1; i < argc; ++i) ok = check_seed(std::strtoull(argv[i], nullptr, 10), 4000) && ok;
  return ok ? 0 : 1;
}
