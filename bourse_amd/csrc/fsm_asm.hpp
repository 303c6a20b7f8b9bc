// fsm_asm.hpp — the draw loop of k_agents_fsm (agents_fsm_body.inc, loop 1), hand-written for gfx950; behind it (further
// down, with their own headers) the kernel's shuffle loop and publish loop, fsm_shuffle_asm and fsm_publish_asm.
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

// ---- the kernel's tail: the Fisher-Yates shuffle (agents_fsm_body.inc, loop 2) and the publish loop behind it, by hand
// (BOURSE_AMD_FSM_TAIL: bit 0 = the shuffle, bit 1 = the publish; 0 = both compiled, as before these statements existed).
// Both sit on the same lone-wave chain as the draw loop.  They use the draw statement's scratch registers (the same
// names; FA_SAVE / FA_LOOP as there) and add no numbered register to the kernel.
//
// Shuffle, 30 instructions per iteration (compiled: 40-41).  Semantics are those of the C++ loop: one next_u32 per
// iteration per lane, rg = i + 1, zn = (rg << clz(rg)) - 1, accept iff lo(x * rg) <= zn, swap list[i] with
// list[hi(x * rg)], --i.  What went:
//   * the two exposed LDS round trips of an accepted iteration: both reads are issued UNPREDICATED as soon as their
//     addresses exist (i is loop-carried; j = hi(x * rg) < rg whether or not the draw is accepted: in bounds for every
//     lane in the loop), the generator's ten-instruction state update runs under their round trip, and ONE
//     s_waitcnt lgkmcnt(0) stands behind it;
//   * the predicated region: the two writes and the update of rg / zn run under exec = ACC (v_cmpx of the acceptance
//     test, AND-ed with the loop's mask by the hardware), then exec is the loop's mask again by a plain s_mov;
//   * the exit test: one v_cmpx into the owned pair FA_LOOP, one branch (no accumulated exit mask);
//   * i itself: only rg = i + 1 is carried (&list[i] = lds_slot0 - 128 + rg * 128), so there are no register copies;
//   * hi(s0 * 5): the draw statement's shift-add, not a second 64-bit multiply.
// The first two instructions of the NEXT draw (they read the updated state only) stand between the exit test's v_cmpx
// and its branch: the loop is rotated by two instructions, which the prologue issues once.
//
// Hazards (nothing inside an asm string is padded):
//   * VALU-written SGPR -> SALU: FA_LOOP is written by v_cmpx and read by the s_mov of exec a whole iteration (29
//     instructions) later; the acceptance v_cmpx writes vcc, which nothing reads;
//   * VALU-written SGPR -> VALU operand: none (the carry-outs and the acceptance mask go to vcc, nothing reads it);
//   * v_cmpx -> s_cbranch_execnz: two vector instructions lie between; v_cmpx -> LDS / VALU under the new exec: interlocked;
//   * SALU write of exec -> VALU: interlocked, no wait states;
//   * LDS executes one wave's operations in order: an iteration's reads see the previous iteration's writes, and a
//     lane whose i == j reads one value twice and writes it twice; the reads' results are waited for inside the
//     statement (lgkmcnt(0) before the writes), and the statement ends with s_waitcnt lgkmcnt(0) because the compiler
//     does not count the writes inside it;
//   * clobbers: the scratch registers by number, vcc, scc, "memory".
#define FS_RG "v216"     // rg = i + 1
#define FS_ZN "v217"     // (rg << clz(rg)) - 1
#define FS_BASE "v210"   // lds_slot0 - 128: &list[i] = FS_BASE + rg * 128
#define FS_AI "v222"     // &list[i]
#define FS_AJ "v220"     // &list[j]
#define FS_VI "v208"     // list[i]
#define FS_VJ "v209"     // list[j]
#define FS_CLZ "v221"

// while (i != 0) { one draw; on acceptance swap list[i], list[hi(x * rg)] and --i }, i = n_ev - 1 (n_ev > 1)
__device__ __forceinline__ void fsm_shuffle_asm(uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1, uint32_t n_ev,
                                                uint32_t lds_slot0) {
  asm volatile(
      "s_mov_b64 " FA_SAVE ", exec\n\t"
      "v_mov_b32 " FS_RG ", %[nev]\n\t"
      "v_ffbh_u32_e32 " FS_CLZ ", %[nev]\n\t"
      "v_add_u32_e32 " FS_BASE ", 0xffffff80, %[slot0]\n\t"
      "v_lshl_add_u32 " FS_ZN ", %[nev], " FS_CLZ ", -1\n\t"
      "v_cmpx_lt_u32_e64 " FA_LOOP ", 1, %[nev]\n\t"
      "v_mad_u64_u32 " FA_P ", vcc, %[a0], 5, 0\n\t"
      "v_lshl_add_u32 " FA_T5 ", %[a1], 2, %[a1]\n\t"
      "s_cbranch_execz .Lfsh_end_%=\n\t"
      ".Lfsh_top_%=:\n\t"
      // the draw x = rotl(s0 * 5, 7) * 9 (its first two instructions stand at the bottom), m = x * rg, the two reads
      "v_lshl_add_u32 " FS_AI ", " FS_RG ", 7, " FS_BASE "\n\t"
      "v_add_u32_e32 " FA_R ", " FA_T5 ", " FA_P1 "\n\t"
      "ds_read_u16 " FS_VI ", " FS_AI "\n\t"
      "v_alignbit_b32 " FA_R ", " FA_P0 ", " FA_R ", 25\n\t"
      "v_lshl_add_u32 " FA_X ", " FA_R ", 3, " FA_R "\n\t"
      "v_mad_u64_u32 " FA_M ", vcc, " FA_X ", " FS_RG ", 0\n\t"
      "v_lshl_add_u32 " FS_AJ ", " FA_VAL ", 7, %[slot0]\n\t"  // j = hi(x * rg) < rg
      "ds_read_u16 " FS_VJ ", " FS_AJ "\n\t"
      // the generator's state update, under the reads' round trip
      "v_xor_b32_e32 " FA_T0 ", %[b0], %[a0]\n\t"
      "v_xor_b32_e32 " FA_T1 ", %[b1], %[a1]\n\t"
      "v_alignbit_b32 " FA_R0 ", %[a0], %[a1], 8\n\t"
      "v_alignbit_b32 " FA_R1 ", %[a1], %[a0], 8\n\t"
      "v_lshlrev_b32_e32 " FA_U0 ", 16, " FA_T0 "\n\t"
      "v_alignbit_b32 " FA_U1 ", " FA_T1 ", " FA_T0 ", 16\n\t"
      "v_alignbit_b32 %[b0], " FA_T1 ", " FA_T0 ", 27\n\t"
      "v_alignbit_b32 %[b1], " FA_T0 ", " FA_T1 ", 27\n\t"
      "v_bitop3_b32 %[a0], " FA_R0 ", " FA_T0 ", " FA_U0 " bitop3:0x96\n\t"
      "v_bitop3_b32 %[a1], " FA_R1 ", " FA_T1 ", " FA_U1 " bitop3:0x96\n\t"
      // exec = ACC: the swap, the next range and its zone
      "v_cmpx_ge_u32_e32 vcc, " FS_ZN ", " FA_MLO "\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "ds_write_b16 " FS_AI ", " FS_VJ "\n\t"
      "ds_write_b16 " FS_AJ ", " FS_VI "\n\t"
      "v_add_u32_e32 " FS_RG ", -1, " FS_RG "\n\t"
      "v_ffbh_u32_e32 " FS_CLZ ", " FS_RG "\n\t"
      "v_lshl_add_u32 " FS_ZN ", " FS_RG ", " FS_CLZ ", -1\n\t"
      "s_mov_b64 exec, " FA_LOOP "\n\t"
      "v_cmpx_lt_u32_e64 " FA_LOOP ", 1, " FS_RG "\n\t"  // i != 0
      "v_mad_u64_u32 " FA_P ", vcc, %[a0], 5, 0\n\t"
      "v_lshl_add_u32 " FA_T5 ", %[a1], 2, %[a1]\n\t"
      "s_cbranch_execnz .Lfsh_top_%=\n\t"
      ".Lfsh_end_%=:\n\t"
      "s_mov_b64 exec, " FA_SAVE "\n\t"
      "s_waitcnt lgkmcnt(0)"
      : [a0] "+v"(a0), [a1] "+v"(a1), [b0] "+v"(b0), [b1] "+v"(b1)
      : [nev] "v"(n_ev), [slot0] "v"(lds_slot0)
      : "s14", "s15", "s16", "s17", "v200", "v201", "v202", "v204", "v205", "v208", "v209", "v210", "v216", "v217", "v218",
        "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", "v228", "vcc", "scc", "memory");
}

// Publish: bt[BT_EV + k / 2] = list[k] | list[k + 1] << 16 for k < n_ev, eight events (one 16-byte store) at a time.
// Compiled it was a 4x-unrolled loop of ~50 instructions per 8 events in which every ds_read_u16 met its own wait or sat
// behind an exec save / restore for the odd-tail test.  Here the full groups (k + 8 <= n_ev) take 19 instructions: eight
// reads, ONE wait, four v_lshl_or, one global_store_dwordx4, no predicate but the loop's mask.  The lane's last, partial
// group (n_ev & 7 events) is stored once behind the loop with the entries at or beyond n_ev written as 0 (the odd tail's
// zero among them): nothing reads a batch entry at or beyond n_ev (k_step_batch's loops run to n_ev and its gathers are
// gated by it; the region holds stale entries of longer earlier lists anyway).  Every read stays inside the lane's 64 R
// list slots and every store inside the 32 R-dword event region: a partial group starts at n_ev & ~7 <= 64 R - 8.
// (ds_read_u16_d16 / _d16_hi are not used: with SRAM ECC, as on this target, a d16 load does not keep the register's
// other half.)
// Hazards (nothing inside an asm string is padded):
//   * v_cmpx -> s_cbranch: every pair has the next group's first read between (the loop is rotated by that one
//     instruction; a read issued under an exec of 0 does nothing, and the tail issues its own);
//   * VALU-written SGPR / vcc -> VALU operand needs 2 wait states: the partial group's six keep-masks are compared into
//     six SGPR pairs of their own (the draw statement's phase-mask pairs, free here) BEFORE the wait for the reads, and
//     each v_cndmask reads its pair six instructions and that wait later; nothing reads vcc, and no select follows its
//     compare directly;
//   * VALU-written SGPR -> SALU: none (FA_LOOP is read by nothing; exec comes back from FA_SAVE, an SALU copy);
//   * a 16-byte store's data registers are not written for 2 wait states behind it (the loop: a dozen instructions; the
//     end: s_nop 1, for the compiler's next instruction);
//   * every read is waited for inside (LDS returns in order: the single wait of a group covers the rotated read too);
//   * the stores are NOT waited for and the compiler does not count them: the statement must be the last memory
//     operation of the kernel's body (agents_fsm_body.inc says so where it calls it);
//   * clobbers: the scratch registers by number, vcc, scc, "memory".
// The eight event words of a group are v200 .. v207.
#define FP_D "v[208:211]"        // the packed group
#define FP_CNT "v212"            // full groups left
#define FP_REM "v213"            // n_ev & 7

// lds = LDS byte address of list[lane], dst = bt + BT_EV (16-byte aligned)
__device__ __forceinline__ void fsm_publish_asm(uint32_t n_ev, uint32_t lds, uint32_t* dst) {
  asm volatile(
      "s_mov_b64 " FA_SAVE ", exec\n\t"
      "v_lshrrev_b32_e32 " FP_CNT ", 3, %[nev]\n\t"
      "v_and_b32_e32 " FP_REM ", 7, %[nev]\n\t"
      "v_cmpx_ne_u32_e64 " FA_LOOP ", 0, " FP_CNT "\n\t"
      "ds_read_u16 v200, %[lds]\n\t"
      "s_cbranch_execz .Lfpb_tail_%=\n\t"
      ".Lfpb_top_%=:\n\t"
      "ds_read_u16 v201, %[lds] offset:128\n\t"
      "ds_read_u16 v202, %[lds] offset:256\n\t"
      "ds_read_u16 v203, %[lds] offset:384\n\t"
      "ds_read_u16 v204, %[lds] offset:512\n\t"
      "ds_read_u16 v205, %[lds] offset:640\n\t"
      "ds_read_u16 v206, %[lds] offset:768\n\t"
      "ds_read_u16 v207, %[lds] offset:896\n\t"
      "v_add_u32_e32 " FP_CNT ", -1, " FP_CNT "\n\t"
      "v_add_u32_e32 %[lds], 0x400, %[lds]\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_lshl_or_b32 v208, v201, 16, v200\n\t"
      "v_lshl_or_b32 v209, v203, 16, v202\n\t"
      "v_lshl_or_b32 v210, v205, 16, v204\n\t"
      "v_lshl_or_b32 v211, v207, 16, v206\n\t"
      "global_store_dwordx4 %[dst], " FP_D ", off\n\t"
      "v_lshl_add_u64 %[dst], %[dst], 0, 16\n\t"
      "v_cmpx_ne_u32_e64 " FA_LOOP ", 0, " FP_CNT "\n\t"
      "ds_read_u16 v200, %[lds]\n\t"  // the next group's first read, between the test and its branch
      "s_cbranch_execnz .Lfpb_top_%=\n\t"
      ".Lfpb_tail_%=:\n\t"
      // the partial group of the lanes that have one
      "s_mov_b64 exec, " FA_SAVE "\n\t"
      "v_cmpx_ne_u32_e64 " FA_LOOP ", 0, " FP_REM "\n\t"
      "ds_read_u16 v200, %[lds]\n\t"
      "s_cbranch_execz .Lfpb_end_%=\n\t"
      "ds_read_u16 v201, %[lds] offset:128\n\t"
      "ds_read_u16 v202, %[lds] offset:256\n\t"
      "ds_read_u16 v203, %[lds] offset:384\n\t"
      "ds_read_u16 v204, %[lds] offset:512\n\t"
      "ds_read_u16 v205, %[lds] offset:640\n\t"
      "ds_read_u16 v206, %[lds] offset:768\n\t"
      // entry k is kept iff k < n_ev & 7: six masks, taken under the reads' round trip, each read 6+ instructions later
      "v_cmp_lt_u32_e64 " FA_PACT ", 1, " FP_REM "\n\t"
      "v_cmp_lt_u32_e64 " FA_PSIDE ", 2, " FP_REM "\n\t"
      "v_cmp_lt_u32_e64 " FA_PTICK ", 3, " FP_REM "\n\t"
      "v_cmp_lt_u32_e64 " FA_PVOL ", 4, " FP_REM "\n\t"
      "v_cmp_lt_u32_e64 " FA_CHIT ", 5, " FP_REM "\n\t"
      "v_cmp_lt_u32_e64 " FA_CACC ", 6, " FP_REM "\n\t"
      "s_waitcnt lgkmcnt(0)\n\t"
      "v_cndmask_b32_e64 v201, 0, v201, " FA_PACT "\n\t"
      "v_cndmask_b32_e64 v202, 0, v202, " FA_PSIDE "\n\t"
      "v_cndmask_b32_e64 v203, 0, v203, " FA_PTICK "\n\t"
      "v_cndmask_b32_e64 v204, 0, v204, " FA_PVOL "\n\t"
      "v_cndmask_b32_e64 v205, 0, v205, " FA_CHIT "\n\t"
      "v_cndmask_b32_e64 v206, 0, v206, " FA_CACC "\n\t"
      "v_lshl_or_b32 v208, v201, 16, v200\n\t"
      "v_lshl_or_b32 v209, v203, 16, v202\n\t"
      "v_lshl_or_b32 v210, v205, 16, v204\n\t"
      "v_mov_b32 v211, v206\n\t"  // (entry 7 of a partial group lies beyond n_ev)
      "global_store_dwordx4 %[dst], " FP_D ", off\n\t"
      ".Lfpb_end_%=:\n\t"
      "s_mov_b64 exec, " FA_SAVE "\n\t"
      "s_nop 1"
      : [lds] "+v"(lds), [dst] "+v"(dst)
      : [nev] "v"(n_ev)
      : "s14", "s15", "s16", "s17", "s18", "s19", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "v200",
        "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "vcc", "scc",
        "memory");
}

}  // namespace bkd
