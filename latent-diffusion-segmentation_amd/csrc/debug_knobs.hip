// ldmseg_debug_set / ldmseg_debug_get: the process-global tuning knobs of experiments, tools and tests as one table, and the
// igemm dispatch log entries that go with them.
#include <cstdio>
#include <cstring>

#include "runtime.h"
#include "vae_bwd.h"

using namespace ldmseg;
using namespace ldmseg::rt;

namespace {

struct Knob {
  int key;
  const char* meaning;
  void (*set)(int);    // null: the key cannot be set ("unknown debug key")
  int (*get)();        // null: the key reads back as 0
  bool replans;        // setting it changes what a workspace plan measures: bumps g_plan_epoch
};

unsigned long long g_ts_ptr = 0;      // keys 3 / 4: the two halves of a device stamp buffer's address
void set_ts_half(unsigned long long keep_mask, unsigned long long bits) {
  g_ts_ptr = (g_ts_ptr & keep_mask) | bits;
  igemm_set_tsbuf((void*)(uintptr_t)g_ts_ptr);
}

// clang-format off
const Knob kKnobs[] = {
  {-1, "igemm: the shipped value of key 1", nullptr, [] { return igemm_default_dbg(); }, false},
  {1, "igemm: tile policy bits (they decide the split-K slice counts, i.e. the size of the partial-sum scratch)", [](int v) { igemm_set_dbg(v); }, [] { return igemm_get_dbg(); }, true},
  {2, "attention.hip: query-fragment choice (attention_set_qf1)", [](int v) { attention_set_qf1(v); }, nullptr, false},
  {3, "igemm: low half of a device stamp buffer's address (ablate builds)", [](int v) { set_ts_half(0xffffffff00000000ull, (unsigned)v); }, nullptr, false},
  {4, "igemm: high half of that address", [](int v) { set_ts_half(0xffffffffull, (unsigned long long)(unsigned)v << 32); }, nullptr, false},
  {5, "igemm: forced entry of the instantiation list, -1 = off (tools/tune_igemm.py)", [](int v) { igemm_force_cfg(v); }, nullptr, true},
  {6, "ldmseg_bench_igemm: weight copies rotated", [](int v) { ops_bench_knob(6, v); }, nullptr, false},
  {7, "ldmseg_bench_igemm: folded-LayerNorm launch", [](int v) { ops_bench_knob(7, v); }, nullptr, false},
  {8, "GroupNorm: kernel variant (bit 3 changes which scratch conv_groupnorm plans)", [](int v) { groupnorm_set_variant(v); }, [] { return groupnorm_knob(8); }, true},
  {9, "igemm: K order of 3x3 conv launches: -1 rule, 0 tap-major, 1 channel-major", [](int v) { igemm_set_cm_mode(v); }, [] { return igemm_get_cm_mode(); }, true},
  {10, "cooperative GroupNorm hand-off, set: mode (1: every workgroup computes its partners' records itself); get: fallback count of the ring regions (ldmseg_op_* launches)",
   [](int v) { groupnorm_set_coop(v, groupnorm_knob(11)); }, [] { const long long n = gn_coop_fallbacks(nullptr); return n > 0x7fffffffll ? 0x7fffffff : (int)n; }, false},
  {11, "cooperative GroupNorm hand-off: poll bound in us", [](int v) { groupnorm_set_coop(groupnorm_knob(10), v); }, [] { return groupnorm_knob(11); }, false},
  {12, "transformer feed-forward fusion: bit 0 MLP, bit 1 + proj_out", [](int v) { mlp_fused_set_mode(v); }, [] { return mlp_fused_get_mode(); }, true},
  {13, "fused feed-forward: bit 8 no start-chunk rotation (bits 0-7: ablate builds)", [](int v) { mlp_fused_set_dbg(v); }, nullptr, false},
  {14, "step tail: bit 0 dedicated conv_out kernel (bf16), bit 1 scheduler step in its epilogue (the implicit-GEMM conv_out it falls back to plans split-K scratch)",
   [](int v) { step_tail_set_mode(v); }, [] { return step_tail_get_mode(); }, true},
  {15, "fp8 attention: 1 = scaled MFMAs where the shape allows (default), 0 = unscaled", [](int v) { attention_mx_set_mode(v); }, [] { return attention_mx_get_mode(); }, true},
  {16, "proj_in -> norm1 -> q|k|v in one launch (bf16, 320 channels); default 1", [](int v) { proj_qkv_set_mode(v); }, [] { return proj_qkv_get_mode(); }, true},
  // (17 was round 5's weight-streaming kernel: measured level with igemm_kernel, now a record under tools/experiments/)
  {19, "1 (default): resnet conv2 + conv_shortcut as one launch (bf16)", [](int v) { igemm_set_xt_mode(v); }, [] { return igemm_get_xt_mode(); }, true},
  {20, "1 (default): ff.net.2 and proj_out of the 640- / 1280-channel transformers as one chained Linear", [](int v) { g_ffp_mode = v ? 1 : 0; }, [] { return g_ffp_mode; }, true},
  {21, "1 (default): upsampler convs as four 2x2 phase convs (bf16)", [](int v) { igemm_set_up4_mode(v); }, [] { return igemm_get_up4_mode(); }, true},
  {22, "GroupNorm folded into the fused transformer entry: 0 off, 1 on, n > 1 on with n pixel chunks", [](int v) { g_gnfold_mode = v < 0 ? 0 : v; }, [] { return g_gnfold_mode; }, true},
  {23, "K slices finished inside the igemm launch (round 6).  bit 0: on (256-row tiles, where it measured faster); bit 1: zero-length partner poll (test: the last arriver "
       "reduces the shares of everybody who gave up); bit 2: resnet conv1 -> norm2 on the maps whose conv runs on those tiles as conv (finished in-launch) + GroupNorm instead "
       "of slabs + the fused finish-GroupNorm launch; bit 3: in-launch finish on every tile form that has the instantiation; bits 8-23: poll bound in microseconds (0 = 200).  "
       "Default 5", [](int v) { igemm_set_cf_mode(v); }, [] { return igemm_get_cf_mode(); }, true},
  {24, "igemm tuning: launch-table override, -1 = off (igemm_set_table_override)", [](int v) { igemm_set_table_override(v); }, nullptr, true},
  {25, "1: ldmseg_sample_loop runs the separate image encoder in every step; default 0 = once per call", [](int v) { g_sepenc_every_step = v ? 1 : 0; }, [] { return g_sepenc_every_step; }, false},
  {26, "weight gradient: CU count handed to the launch chooser, 0 = the device's (tests: workgroups that walk several items)", [](int v) { wgrad_set_cus(v); }, [] { return wgrad_get_cus(); }, false},
};
// clang-format on

const Knob* find_knob(int key) {
  for (const Knob& k : kKnobs)
    if (k.key == key) return &k;
  return nullptr;
}

}  // namespace

extern "C" {

int ldmseg_debug_set(int key, int value) {
  const Knob* k = find_knob(key);
  if (!k || !k->set) return fail(LDMSEG_E_ARG, "unknown debug key");
  k->set(value);
  if (k->replans) ++g_plan_epoch;
  return 0;
}

int ldmseg_debug_get(int key) {
  const Knob* k = find_knob(key);
  return k && k->get ? k->get() : 0;
}

// "igemm<bf16,BM,BN,WM,WN,NST,PIPE,LDR>[/splitk] splits=S grid=G" of the most recent igemm launch
int ldmseg_igemm_last_kernel(char* buf, int n) {
  if (!buf || n < 1) return LDMSEG_E_ARG;
  std::snprintf(buf, (size_t)n, "%s", igemm_dispatch_line(igemm_last_dispatch()).c_str());
  return 0;
}
int ldmseg_igemm_log(int enable) { igemm_log_enable(enable); return 0; }
int ldmseg_igemm_log_read(char* buf, int n) {
  if (!buf || n < 1) return LDMSEG_E_ARG;
  const std::string s = igemm_log_read();
  if ((int)s.size() + 1 > n) return LDMSEG_E_ARG;
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return 0;
}

}  // extern "C"
