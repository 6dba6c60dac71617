// ws_dbg_host.h — host side of the measurement build (-DUNETPP_WS_DBG=1: in-kernel phase stamps and ablations of the
// wave-specialised conv, scripts/ws_ablate.sh and ws_stamps.sh).  run_conv (unetpp_abi.hip) calls ws_dbg_before_launch and
// ws_dbg_after_launch around the launch and forward_impl calls ws_dbg_end_of_pass; the product build compiles none of this.
//   UNETPP_WS_DBG=bits        phases of conv3x3_ws_kernel switched off (results are garbage)
//   UNETPP_WS_DBG_ONLY=layer  the ablation applies to that launch alone
//   UNETPP_WS_STAMPS=layer    print that launch's in-kernel phase times; "all": one wall-clock timeline of the forward
#pragma once
#ifdef UNETPP_WS_DBG
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "conv3x3_mfma.h"

namespace unetpp {

struct WsDbgPass {
  std::vector<std::string> timeline;      // UNETPP_WS_STAMPS=all: the wave-specialised launches of this pass, in order
  bool stamp_this = false;                // the launch in flight is the one UNETPP_WS_STAMPS names
};

inline unsigned long long*& ws_dbg_stamp_buf() {
  static unsigned long long* buf = nullptr;
  return buf;
}

// Before a conv launch: the ablation bits and the stamp buffer of `layer` go into its arguments.
inline void ws_dbg_before_launch(WsDbgPass& d, ConvArgs& a, const std::string& layer, hipStream_t s) {
  { const char* v = getenv("UNETPP_WS_DBG"); a.dbg = v ? atoi(v) : 0; }
  // UNETPP_WS_DBG_ONLY=layer: the ablation applies to that launch alone -- its inputs stay genuine (a layer fed with the
  // zeros an ablated predecessor leaves behind runs at a different clock)
  { const char* only = getenv("UNETPP_WS_DBG_ONLY"); if (only && layer != only) a.dbg = 0; }
  unsigned long long*& stamp_buf = ws_dbg_stamp_buf();
  const char* stamp_layer = getenv("UNETPP_WS_STAMPS");      // layer name: print that launch's in-kernel phase times
  const bool stamp_all = stamp_layer && !strcmp(stamp_layer, "all");      // "all": one wall-clock timeline of the forward
  d.stamp_this = stamp_layer && layer == stamp_layer;
  if (d.stamp_this || stamp_all) {
    if (!stamp_buf) { (void)hipMalloc((void**)&stamp_buf, (size_t)32 * 1024 * 32 * 8); (void)hipMemset(stamp_buf, 0, (size_t)32 * 1024 * 32 * 8); }
    if (d.stamp_this) (void)hipMemsetAsync(stamp_buf, 0, 1024 * 32 * 8 * 5, s);
    a.stamps = stamp_buf + (stamp_all ? (size_t)(1 + d.timeline.size()) * 1024 * 32 : 0);
    if (stamp_all) d.timeline.push_back(layer);
  }
}

// After the launch of the layer UNETPP_WS_STAMPS names (wave-specialised kernel only): its phase times, on the fourth call.
inline void ws_dbg_after_launch(const WsDbgPass& d, const ConvArgs& a, const std::string& layer, bool ws, hipStream_t s) {
  if (!d.stamp_this || !ws) return;
  static int printed = 0;
  std::vector<unsigned long long> hs(1024 * 32 * 5);
  (void)hipStreamSynchronize(s);
  (void)hipMemcpy(hs.data(), ws_dbg_stamp_buf(), hs.size() * 8, hipMemcpyDeviceToHost);
  if (printed++ != 3) return;      // a warm launch
  double sum[32] = {0};
  int nwg = 0;
  for (int b = 0; b < 1024; ++b) { if (!hs[b * 32 + 1] && !hs[b * 32 + 16]) continue; ++nwg; for (int i = 0; i < 32; ++i) sum[i] += (double)hs[b * 32 + i]; }
  fprintf(stderr, "[stamps %s] %d workgroups, mean cycles per workgroup:\n  consumer: barrier %.0f  chunks %.0f  epilogue %.0f  init %.0f\n"
                  "  producer: skip issue %.0f wait %.0f barrier %.0f | up issue %.0f interp %.0f (reads %.0f arithmetic %.0f split+stores %.0f)"
                  " wait %.0f barrier %.0f | setup %.0f\n", layer.c_str(), nwg,
          sum[0] / nwg, sum[1] / nwg, sum[2] / nwg, sum[3] / nwg, sum[16] / nwg, sum[17] / nwg, sum[18] / nwg, sum[19] / nwg, sum[20] / nwg,
          sum[24] / nwg, sum[25] / nwg, sum[26] / nwg, sum[21] / nwg, sum[22] / nwg, sum[23] / nwg);
  // wall-clock (100 MHz) begin / end of consumer wave 0 of every workgroup, relative to the earliest begin
  std::vector<double> bg, en;
  unsigned long long t0 = ~0ull;
  std::vector<double> cb, pe;
  for (int b = 0; b < 1024; ++b) if (hs[b * 32 + 6]) t0 = std::min(t0, hs[b * 32 + 6]);
  for (int b = 0; b < 1024; ++b) if (hs[b * 32 + 6]) {
    bg.push_back((hs[b * 32 + 6] - t0) * 0.01); en.push_back((hs[b * 32 + 5] - t0) * 0.01);
    cb.push_back((hs[b * 32 + 4] - t0) * 0.01); pe.push_back((hs[b * 32 + 16 + 12] - t0) * 0.01);
  }
  std::sort(bg.begin(), bg.end()); std::sort(en.begin(), en.end()); std::sort(cb.begin(), cb.end()); std::sort(pe.begin(), pe.end());
  if (!bg.empty()) fprintf(stderr, "  consumer loop begins p50 %.2f max %.2f | producer wave 0 ends p50 %.2f max %.2f\n", cb[cb.size() / 2], cb.back(), pe[pe.size() / 2], pe.back());
  if (a.dbg & WS_EVENT_LOG)
    for (int b : {0, 1, 100, 200}) {      // event logs of consumer wave 0 and producer wave 0 (phase:us after the earliest kernel entry)
      for (int role = 0; role < 2; ++role) {
        fprintf(stderr, "  wg %3d %s:", b, role ? "producer" : "consumer");
        const unsigned long long* ev = hs.data() + 1024 * 32 + ((size_t)b * 2 + role) * 64;
        for (int i = 0; i < 60 && ev[i]; ++i) fprintf(stderr, " %d:%.2f", (int)(ev[i] >> 56), (double)((ev[i] & 0xffffffffffffffull) - t0) * 0.01);
        fprintf(stderr, "\n");
      }
    }
  if (!bg.empty())
    fprintf(stderr, "  wall clock (us after the first workgroup's kernel entry): entry p50 %.2f p90 %.2f max %.2f | end min %.2f p50 %.2f p90 %.2f max %.2f\n",
            bg[bg.size() / 2], bg[bg.size() * 9 / 10], bg.back(), en.front(), en[en.size() / 2], en[en.size() * 9 / 10], en.back());
}

// After a pass under UNETPP_WS_STAMPS=all, on the sixth: wall-clock (100 MHz, chip-wide) entry of the first workgroup and end of
// the last consumer-0 / producer-0 wave of every wave-specialised launch, relative to the first launch's entry: what lies
// between the launches.
inline void ws_dbg_end_of_pass(const WsDbgPass& d, hipStream_t s) {
  if (d.timeline.empty()) return;
  static int pass = 0;
  if (++pass != 6) return;
  (void)hipStreamSynchronize(s);
  std::vector<unsigned long long> hs((size_t)(1 + d.timeline.size()) * 1024 * 32);
  (void)hipMemcpy(hs.data(), ws_dbg_stamp_buf(), hs.size() * 8, hipMemcpyDeviceToHost);
  unsigned long long T0 = ~0ull;
  double prev_end = 0;
  for (size_t li = 0; li < d.timeline.size(); ++li) {
    const unsigned long long* r = hs.data() + (1 + li) * 1024 * 32;
    unsigned long long first = ~0ull, last = 0; int nwg = 0;
    for (int b = 0; b < 1024; ++b) if (r[b * 32 + 6]) { ++nwg; first = std::min(first, r[b * 32 + 6]); last = std::max(last, std::max(r[b * 32 + 5], r[b * 32 + 16 + 12])); }
    if (!nwg) continue;
    if (T0 == ~0ull) T0 = first;
    const double b0 = (first - T0) * 0.01, e0 = (last - T0) * 0.01;
    fprintf(stderr, "[timeline] %-16s %4d wg  entry %8.2f  end %8.2f  inside %6.2f  since previous end %6.2f\n", d.timeline[li].c_str(), nwg, b0, e0, e0 - b0, b0 - prev_end);
    prev_end = e0;
  }
}

}  // namespace unetpp
#endif  // UNETPP_WS_DBG
