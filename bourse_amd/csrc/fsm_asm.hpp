// fsm_asm.hpp — the draw loop of k_agents_fsm (agents_fsm_body.inc, loop 1), hand-written for gfx950.
//
// Why assembly: k_agents_fsm is ONE dependent chain per wave (one wave per SIMD, ~470 draws per step) and the split
// pipeline's step time is the cycle of one part: this chain plus the part's k_step_batch.  A lone wave
// issues one instruction per ~4.4 clocks whatever its kind, so the chain's length IS the instruction count of a draw.
// The compiled loop takes 66; every attempt to shorten it in C++ came back longer (docs/EXPERIMENTS.md).  Written by
// hand the same draw takes 55.  What went:
//   * the two predicated regions (list append under QUEUE, new-order store under A_VOL): save-exec + skip branch +
//     restore each.  The append needs no predicate at all - the lane's next free list slot list[n_ev] is written on
//     EVERY draw (n_ev <= n < 64 R: in bounds; a word that is not queued is overwritten by the next one or lies behind
//     n_ev, never read) - and the store is bracketed by two plain writes of exec: A_VOL, then the loop's own mask;
//   * the exit test: v_cmpx writes the loop's mask to exec AND to an SGPR pair the statement owns (inactive lanes
//     compare as 0, so the result IS the new mask: no accumulating s_or / s_andn2), one branch at the bottom;
//   * the live test: the segment's live word arrives BIT-REVERSED, so bit (n & 63) is the sign of (w << n): a shift and
//     a compare instead of shift, and, compare;
//   * the event word: every draw's value is taken with 2 added ((x * range + (2 << 32)) >> 32: the multiply-add's free
//     addend), so the side kept for the word is 2 | side and n | EV_NEW | side << 14 is ONE v_lshl_or_b32; the statement
//     starts from tick_lo - 2 and vol_lo - 2, which gives the same price and volume (arithmetic mod 2^32);
//   * hi(s0 * 5): shift-add of a1 beside the low multiply instead of a register copy and a second 64-bit multiply;
//   * the pv address: n is kept in a register pair whose high half is 0, so it is one v_lshl_add_u64;
//   * cur_side / cur_price are taken under the PHASE masks (a rejected draw's value is overwritten by the accepted
//     one before the phase is left), so A_SIDE / A_TICK are needed for the phase algebra only.
//
// Semantics are those of the C++ loop (BOURSE_AMD_FSM_ASM = 0, and BK_PB = 1 always): one next_u32 per draw per lane,
// the same acceptance tests, event words, pv[n] = {price, vol_lo + val}, the same order of list appends.
//
// Hazards the ordering relies on (nothing inside an asm string is padded):
//   * a VALU-written SGPR (the three v_cmp masks) read by the SCALAR unit is interlocked but stalls a lone wave ~16
//     clocks when read at once: the first s_and of a draw comes 15+ vector instructions after the last v_cmp;
//   * VALU-written SGPR -> VALU operand needs 2 wait states: no vector instruction reads such a register (the compare
//     masks go through the scalar algebra first; the carry-outs go to vcc, which nothing reads);
//   * v_cmpx -> s_cbranch_execnz: three SALU instructions lie between; the s_mov of exec from the owned copy of the
//     loop mask reads a register written a whole iteration earlier;
//   * SALU writes of exec / of a mask -> VALU, VMEM: interlocked, no wait states;
//   * LDS: the writes carry no register result, and LDS executes one wave's operations in order, so loop 2 reads what
//     was appended; the statement still ends with s_waitcnt lgkmcnt(0) because the compiler does not count the writes
//     inside it and its own counted waits behind the statement must not be off;
//   * global_store_dwordx2: 64-bit data, not the wider-store hazard; pv is never read back in this kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bkd {

// fixed scratch registers of the statement (declared as clobbers), named in one place
// SGPR pairs: wave masks (s32 / s33 are left out: the compiler reserves s32)
#define FA_SAVE "s[14:15]"   // exec at entry
#define FA_LOOP "s[16:17]"   // lanes still in the loop (the statement's copy of exec)
#define FA_PACT "s[18:19]"   // phase masks, one-hot per lane
#define FA_PSIDE "s[20:21]"
#define FA_PTICK "s[22:23]"
#define FA_PVOL "s[24:25]"
#define FA_CHIT "s[26:27]"   // C_HIT, then HIT, then A_TICK
#define FA_CACC "s[28:29]"   // C_ACC
#define FA_CLIVE "s[30:31]"  // C_LIVE, then TO_SIDE
#define FA_Q "s[34:35]"      // CANCEL, then QUEUE, then A_SIDE
#define FA_AVOL "s[36:37]"   // A_VOL
// VGPRs (below the kernel's claim BOURSE_AMD_FSM_TOP_VGPR: they add nothing to its footprint)
#define FA_P2 "v[196:197]"  // (tick_lo - 2) * tick_size (low word; the high one is not used)
#define FA_M2 "v198"        // -2, then vol_lo - 2
#define FA_P "v[200:201]"   // s0.lo * 5
#define FA_P0 "v200"
#define FA_P1 "v201"
#define FA_XX "v[202:203]"  // the draw x, zero-extended (v203 = 0)
#define FA_X "v202"
#define FA_XZ "v203"
#define FA_M "v[204:205]"   // x * range + (2 << 32)
#define FA_MLO "v204"
#define FA_VAL "v205"       // val + 2
#define FA_NN "v[206:207]"  // n, zero-extended (v207 = 0)
#define FA_N "v206"
#define FA_NZ "v207"
#define FA_PV "v[208:209]"  // the new order: {cur_price, vol}
#define FA_PRICE "v208"
#define FA_VOL "v209"
#define FA_PR "v[210:211]"  // (val + 2) * tick_size + (tick_lo - 2) * tick_size
#define FA_PRLO "v210"
#define FA_T "v[212:213]"   // reversed live word << n
#define FA_THI "v213"
#define FA_PA "v[214:215]"  // &pv[n]
#define FA_RANGE "v216"
#define FA_ZONE "v217"
#define FA_T5 "v218"        // s0.hi * 5
#define FA_R "v219"
#define FA_SIDE "v220"      // 2 | side of the order being drawn
#define FA_WORD "v221"
#define FA_LADDR "v222"
#define FA_T0 "v223"
#define FA_T1 "v224"
#define FA_R0 "v225"
#define FA_R1 "v226"
#define FA_U0 "v227"
#define FA_U1 "v228"
#define FA_ZMAX "v229"      // 0x7FFFFFFF: the zone of range 2
#define FA_ADD "v[230:231]" // 2 << 32
#define FA_ADDLO "v230"
#define FA_ADDHI "v231"

// One segment of one group: while (n < send) { one draw }.  wrev = the segment's live word, bit-reversed; lds_slot0 =
// LDS byte address of list[lane]; price0 = tick_lo * tick_size (the statement takes 2 tick sizes off it, and 2 off vol_lo).
__device__ __forceinline__ void fsm_draw_asm(uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1, uint32_t& n,
                                             uint32_t& n_ev, uint32_t trng, uint32_t vrng, uint32_t tzone, uint32_t vzone,
                                             uint32_t lds_slot0, uint64_t wrev, uint2* pv, uint64_t price0,
                                             uint64_t thr8, uint32_t tick_size, uint32_t vol_lo, uint32_t send) {
  asm volatile(
      "s_mov_b64 " FA_SAVE ", exec\n\t"
      "s_mov_b64 " FA_PACT ", -1\n\t"
      "s_mov_b64 " FA_PSIDE ", 0\n\t"
      "s_mov_b64 " FA_PTICK ", 0\n\t"
      "s_mov_b64 " FA_PVOL ", 0\n\t"
      "v_mov_b32 " FA_N ", %[n]\n\t"
      "v_mov_b32 " FA_NZ ", 0\n\t"
      "v_mov_b32 " FA_XZ ", 0\n\t"
      "v_mov_b32 " FA_ADDLO ", 0\n\t"
      "v_mov_b32 " FA_ADDHI ", 2\n\t"
      "v_bfrev_b32 " FA_ZMAX ", -2\n\t"
      "v_mov_b32 " FA_SIDE ", 0\n\t"
      "v_mov_b32 " FA_PRICE ", 0\n\t"
      "v_mov_b32 " FA_M2 ", -2\n\t"
      "v_mad_u64_u32 " FA_P2 ", vcc, " FA_M2 ", %[tick], %[price0]\n\t"
      "v_add_u32_e32 " FA_M2 ", %[vol], " FA_M2 "\n\t"
      "v_cmpx_gt_u32_e64 " FA_LOOP ", %[send], " FA_N "\n\t"
      "s_cbranch_execz .Lfsm_end_%=\n\t"
      ".Lfsm_top_%=:\n\t"
      // the draw: x = rotl(s0 * 5, 7) * 9 (low word); the live test and the phase's range / zone beside it
      "v_mad_u64_u32 " FA_P ", vcc, %[a0], 5, 0\n\t"
      "v_lshl_add_u32 " FA_T5 ", %[a1], 2, %[a1]\n\t"
      "v_lshlrev_b64 " FA_T ", " FA_N ", %[wrev]\n\t"
      "v_cndmask_b32_e64 " FA_RANGE ", %[vrng], %[trng], " FA_PTICK "\n\t"
      "v_cndmask_b32_e64 " FA_ZONE ", %[vzone], %[tzone], " FA_PTICK "\n\t"
      "v_add_u32_e32 " FA_R ", " FA_T5 ", " FA_P1 "\n\t"
      "v_cndmask_b32_e64 " FA_RANGE ", " FA_RANGE ", 2, " FA_PSIDE "\n\t"
      "v_alignbit_b32 " FA_R ", " FA_P0 ", " FA_R ", 25\n\t"
      "v_cndmask_b32_e64 " FA_ZONE ", " FA_ZONE ", " FA_ZMAX ", " FA_PSIDE "\n\t"
      "v_lshl_add_u32 " FA_X ", " FA_R ", 3, " FA_R "\n\t"
      "v_cmp_gt_i32_e64 " FA_CLIVE ", 0, " FA_THI "\n\t"
      "v_mad_u64_u32 " FA_M ", vcc, " FA_X ", " FA_RANGE ", " FA_ADD "\n\t"
      "v_cmp_gt_u64_e64 " FA_CHIT ", %[thr8], " FA_XX "\n\t"
      // the generator's state update (10 instructions that depend on no predicate), the rest of the draw among them
      "v_xor_b32_e32 " FA_T0 ", %[b0], %[a0]\n\t"
      "v_cmp_ge_u32_e64 " FA_CACC ", " FA_ZONE ", " FA_MLO "\n\t"
      "v_xor_b32_e32 " FA_T1 ", %[b1], %[a1]\n\t"
      "v_mad_u64_u32 " FA_PR ", vcc, " FA_VAL ", %[tick], " FA_P2 "\n\t"
      "v_alignbit_b32 " FA_R0 ", %[a0], %[a1], 8\n\t"
      "v_alignbit_b32 " FA_R1 ", %[a1], %[a0], 8\n\t"
      "v_lshlrev_b32_e32 " FA_U0 ", 16, " FA_T0 "\n\t"
      "v_alignbit_b32 " FA_U1 ", " FA_T1 ", " FA_T0 ", 16\n\t"
      "v_alignbit_b32 %[b0], " FA_T1 ", " FA_T0 ", 27\n\t"
      "v_alignbit_b32 %[b1], " FA_T0 ", " FA_T1 ", 27\n\t"
      "v_bitop3_b32 %[a0], " FA_R0 ", " FA_T0 ", " FA_U0 " bitop3:0x96\n\t"
      "v_bitop3_b32 %[a1], " FA_R1 ", " FA_T1 ", " FA_U1 " bitop3:0x96\n\t"
      "v_add_u32_e32 " FA_VOL ", " FA_M2 ", " FA_VAL "\n\t"
      "v_cndmask_b32_e64 " FA_SIDE ", " FA_SIDE ", " FA_VAL ", " FA_PSIDE "\n\t"
      "v_cndmask_b32_e64 " FA_PRICE ", " FA_PRICE ", " FA_PRLO ", " FA_PTICK "\n\t"
      "v_lshl_add_u32 " FA_LADDR ", %[nev], 7, %[slot0]\n\t"
      "v_lshl_add_u64 " FA_PA ", " FA_NN ", 3, %[pv]\n\t"
      // the masks of this draw (scalar algebra), the list append, the new-order store
      "s_and_b64 " FA_CHIT ", " FA_PACT ", " FA_CHIT "\n\t"       // HIT
      "s_and_b64 " FA_AVOL ", " FA_CACC ", " FA_PVOL "\n\t"       // A_VOL
      "s_and_b64 " FA_Q ", " FA_CHIT ", " FA_CLIVE "\n\t"         // CANCEL
      "s_andn2_b64 " FA_CLIVE ", " FA_CHIT ", " FA_CLIVE "\n\t"   // TO_SIDE
      "s_or_b64 " FA_Q ", " FA_Q ", " FA_AVOL "\n\t"              // QUEUE
      "v_lshl_or_b32 " FA_WORD ", " FA_SIDE ", 14, " FA_N "\n\t"  // n | EV_NEW | side << 14
      "s_and_b64 " FA_CHIT ", " FA_CACC ", " FA_PTICK "\n\t"      // A_TICK
      "v_cndmask_b32_e64 " FA_WORD ", " FA_N ", " FA_WORD ", " FA_AVOL "\n\t"
      "v_addc_co_u32_e64 %[nev], vcc, 0, %[nev], " FA_Q "\n\t"    // n_ev += QUEUE
      "ds_write_b16 " FA_LADDR ", " FA_WORD "\n\t"
      "s_and_b64 " FA_Q ", " FA_CACC ", " FA_PSIDE "\n\t"         // A_SIDE (QUEUE has been used)
      "s_mov_b64 exec, " FA_AVOL "\n\t"
      "global_store_dwordx2 " FA_PA ", " FA_PV ", off\n\t"
      "s_andn2_b64 " FA_PACT ", " FA_PACT ", " FA_CLIVE "\n\t"
      "s_or_b64 " FA_PACT ", " FA_PACT ", " FA_AVOL "\n\t"        // ADV = the next P_ACT
      "s_mov_b64 exec, " FA_LOOP "\n\t"
      "v_addc_co_u32_e64 " FA_N ", vcc, 0, " FA_N ", " FA_PACT "\n\t"  // n += ADV
      "s_andn2_b64 " FA_PSIDE ", " FA_PSIDE ", " FA_CACC "\n\t"
      "s_andn2_b64 " FA_PTICK ", " FA_PTICK ", " FA_CACC "\n\t"
      "s_andn2_b64 " FA_PVOL ", " FA_PVOL ", " FA_CACC "\n\t"
      "v_cmpx_gt_u32_e64 " FA_LOOP ", %[send], " FA_N "\n\t"
      "s_or_b64 " FA_PSIDE ", " FA_PSIDE ", " FA_CLIVE "\n\t"
      "s_or_b64 " FA_PTICK ", " FA_PTICK ", " FA_Q "\n\t"
      "s_or_b64 " FA_PVOL ", " FA_PVOL ", " FA_CHIT "\n\t"
      "s_cbranch_execnz .Lfsm_top_%=\n\t"
      ".Lfsm_end_%=:\n\t"
      "s_mov_b64 exec, " FA_SAVE "\n\t"
      "v_mov_b32 %[n], " FA_N "\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [a0] "+v"(a0), [a1] "+v"(a1), [b0] "+v"(b0), [b1] "+v"(b1), [n] "+v"(n), [nev] "+v"(n_ev)
      : [trng] "v"(trng), [vrng] "v"(vrng), [tzone] "v"(tzone), [vzone] "v"(vzone), [slot0] "v"(lds_slot0),
        [wrev] "v"(wrev), [pv] "v"(pv), [price0] "v"(price0), [thr8] "s"(thr8), [tick] "s"(tick_size),
        [vol] "s"(vol_lo), [send] "s"(send)
      : "s14", "s15", "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29",
        "s30", "s31", "s34", "s35", "s36", "s37", "v196", "v197", "v198", "v200", "v201", "v202", "v203", "v204", "v205",
        "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219",
        "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "vcc", "scc", "memory");
}

}  // namespace bkd
