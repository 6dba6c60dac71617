// ws_dbg_dev.h — device side of the measurement build (-DUNETPP_WS_DBG=1; host side: ws_dbg_host.h): the ablation bits of
// ConvArgs::dbg / TapmmArgs::dbg and the hooks the wave-specialised kernels (conv3x3_ws.h, tapmm_ws.h) and pack_store_rows8
// call.  In a product build every hook expands to nothing or to `false`, and the code it guards is dead.
// The hooks are macros: they declare and use names of the role they stand in (a = the kernel's ConvArgs, lane, st_sum, st_t,
// ev_ptr).  scripts/kernel_diff.py checks that an edit here or at a call site leaves both builds' instructions as they were.
#pragma once

namespace unetpp {

// UNETPP_WS_DBG=<sum of bits> (scripts/ws_ablate.sh): phases of conv3x3_ws_kernel switched off or altered.  Results are garbage.
enum WsDbgBit : int {
  WS_NO_INTERP = 1,             // producers, fused upsample: no interpolation (up_rounds)
  WS_NO_HALO_DMA = 2,           // producers: no halo DMA and no low-res-record DMA
  WS_NO_MFMA = 4,               // consumers: fragment reads without their MFMAs
  WS_NO_SLAB_DMA = 8,           // producers: no weight-slab DMA
  WS_NO_CHUNK = 16,             // consumers: no chunk body at all, the barriers only
  WS_NO_RD_SWAP = 32,           // interpolation: corner reads in the old (2-way conflicting) order
  WS_NO_UP_STORE = 64,          // interpolation without its split and LDS stores
  WS_NO_HANDOFF_EPI = 128,      // producers: no epilogue of the handed-over accumulator pair
  WS_NO_EPILOGUE = 256,         // consumers: no epilogue
  WS_NO_CORNER_READ = 512,      // interpolation on constants instead of its corner reads
  WS_PRIO_PROD = 10,            // BIT POSITION: bits 10-11 = s_setprio level of the producer waves
  WS_PRIO_CONS = 12,            // BIT POSITION: bits 12-13 = s_setprio level of the consumer waves
  WS_UNITS_ON_LANES = 16384,    // halo DMA with a pixel's units on neighbouring lanes
  WS_STAMP_INNER = 32768,       // stamps inside the interpolation (WS_STAMP_IN; scripts/ws_stamps.sh)
  WS_NO_CROSS = 65536,          // EXACT8 consumers: no cross-term MFMAs (how much of a chunk they are)
  WS_EVENT_LOG = 131072,        // event log of one wave per role (WS_EVT; single-layer stamps only; printed by ws_dbg_host.h)
  WS_EPI_NO_STORE = 262144,     // epilogue without its global stores (pack_store_rows8)
  WS_EPI_COALESCED = 524288,    // epilogue stores one contiguous KB per instruction (wrong placement; pack_store_rows8)
};
// UNETPP_TAPMM_DBG=<sum of bits>: the same for tapmm_ws_kernel
enum TapmmDbgBit : int {
  TAPMM_NO_DMA = 1,             // producers: no stage DMA
  TAPMM_NO_MFMA = 2,            // consumers: no MFMAs
  TAPMM_NO_STORE = 4,           // consumers: no Y stores
};

}  // namespace unetpp

#ifdef UNETPP_WS_DBG
// is `bit` set in the debug word?  (`word` names a member only measurement builds have: a->dbg, a.dbg)
#define WS_OFF(word, bit) (((word) & (bit)) != 0)
// const wall-clock time stamp (100 MHz, one clock for the whole chip): kernel entry, table staged, role begin
#define WS_WALLCLOCK(name) const unsigned long long name = __builtin_amdgcn_s_memrealtime();
// s_setprio from the two bits at position `pos` of the debug word
#define WS_PRIO(pos) { const int pr_ = (a->dbg >> (pos)) & 3; if (pr_ == 1) __builtin_amdgcn_s_setprio(1); \
                       else if (pr_ == 2) __builtin_amdgcn_s_setprio(2); else if (pr_ == 3) __builtin_amdgcn_s_setprio(3); }
// Role begin: the cycle sums of the role's phases, the time of the last stamp (t0), the role's wall-clock begin (wall0; 0: not
// recorded) and the event pointer of wave 0 of the role (role 0 consumers, 1 producers): 60 events (phase << 56 | wall clock)
// behind the sums, the kernel's entry first.
#define WS_ROLE_BEGIN(role, wave0, t0, wall0) \
  unsigned long long st_sum[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; \
  unsigned long long st_t = (t0); \
  const unsigned long long rt_role = (wall0); \
  unsigned long long* ev_ptr = (a->stamps && WS_OFF(a->dbg, WS_EVENT_LOG) && lane == 0 && blockIdx.x < 1024) \
                                   ? a->stamps + (size_t)1024 * 32 + ((size_t)blockIdx.x * 2 + (role)) * 64 : nullptr; \
  unsigned long long* const ev_end = ev_ptr + 60; \
  if (ev_ptr) *ev_ptr++ = (63ull << 56) | rt_entry; \
  if (!(wave0)) ev_ptr = nullptr;
#define WS_CYCLES __builtin_readcyclecounter()
#define WS_WALL __builtin_amdgcn_s_memrealtime()
#define WS_RESTART st_t = WS_CYCLES;
// event i at a time taken earlier (the first few of a log: no bound test) / now
#define WS_EVT_AT(i, t) { if (ev_ptr) *ev_ptr++ = ((unsigned long long)(i) << 56) | (t); }
#define WS_EVT_AT2(i, t, j, u) { if (ev_ptr) { *ev_ptr++ = ((unsigned long long)(i) << 56) | (t); *ev_ptr++ = ((unsigned long long)(j) << 56) | (u); } }
#define WS_EVT(i) { if (ev_ptr && ev_ptr < ev_end) *ev_ptr++ = ((unsigned long long)(i) << 56) | __builtin_amdgcn_s_memrealtime(); }
// phase i ends here: its cycles since the last stamp, and an event
#define WS_STAMP(i) { const unsigned long long now_ = WS_CYCLES; st_sum[i] += now_ - st_t; st_t = now_; WS_EVT(i) }
// the same inside the interpolation, behind its LDS traffic (WS_STAMP_INNER only)
#define WS_STAMP_IN(i) if (WS_OFF(a->dbg, WS_STAMP_INNER)) { __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); WS_STAMP(i) __builtin_amdgcn_sched_barrier(0); }
// Role end: wave 0 of the role writes its n sums, what `more` puts (WS_PUT) and the end time into slot `end` of
// a->stamps[workgroup][role][16]
#define WS_PUT(role, slot, v) a->stamps[((size_t)blockIdx.x * 2 + (role)) * 16 + (slot)] = (v);
#define WS_ROLE_END(role, wave0, n, end, more) \
  if (a->stamps && (wave0) && lane == 0) { \
    _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) WS_PUT(role, i_, st_sum[i_]) \
    more WS_PUT(role, end, __builtin_amdgcn_s_memrealtime()) }
#else
#define WS_OFF(word, bit) false
#define WS_WALLCLOCK(name)
#define WS_PRIO(pos)
#define WS_ROLE_BEGIN(role, wave0, t0, wall0)
#define WS_RESTART
#define WS_EVT_AT(i, t)
#define WS_EVT_AT2(i, t, j, u)
#define WS_EVT(i) {}
#define WS_STAMP(i) {}
#define WS_STAMP_IN(i) {}
#define WS_ROLE_END(role, wave0, n, end, more)
#endif
