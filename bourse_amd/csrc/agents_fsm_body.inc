// agents_fsm_body.inc - the body of k_agents_fsm (book_device.hpp), included by the uniform kernel with BK_PB = 0 and
// by its per-unit form (bk_set_random_agents_per_book) with BK_PB = 1.  Included rather than called so that the uniform
// kernel compiles exactly as it did when this was its own source (see mixed_lanes_body.inc).
// BK_PB = 1: a lane's groups are its unit's row of the table (u = b: table[u * n_groups + g]), as vector registers;
// only the group sizes stay wave-uniform (DevArgs::groups).  The includer declares fsm_lds, the kernel's dynamic LDS.
// BK_FSM_HAND = 1 (uniform kernel only): loop 1's draw loop is the hand-written statement of fsm_asm.hpp, and with
// BOURSE_AMD_FSM_TAIL so are the shuffle (bit 0) and the publish loop (bit 1).
  uint16_t* list = reinterpret_cast<uint16_t*>(fsm_lds);  // event list of lane l: list[k * 64 + l], 64 * R * 64 entries
  // (which agents place, and on which side, is not tracked here: the event words say it - bit 15 New, bit 14 bid - and
  // k_step_batch rebuilds the masks from them with four LDS atomics per book instead of two per new order in this loop)
  const int lane = threadIdx.x;
  // This kernel is a dependent chain of ~600 iterations on ONE wave per SIMD, co-resident with up to 7 waves of the
  // issue-bound event kernel of another part: top issue priority lets the chain run at its lone-wave pace (the part's
  // next k_step_batch cannot start before it ends) at no cost to the event kernel's throughput
  __builtin_amdgcn_s_setprio(3);
  // ... and it CLAIMS far more VGPRs than it uses (34): the chain is VALU-latency bound, and every k_step_batch wave
  // sharing its SIMD's VALU stretches it (151 us alone, 185-194 us under 8 event waves).  A 232-VGPR footprint leaves
  // room for 7 event waves beside one of these waves and 1 beside two of them, instead of 8 and 8; measured on C3
  // (profiles/r02/fsm_vgpr_sweep.txt): no pad 184 M, 104: 198, 168: 214, 200-264: 215-220 (plateau), 296: 169 M
  // book-steps/s (from 296 up the dispatcher cannot place these waves until a whole SIMD drains).
#if BOURSE_AMD_FSM_TOP_VGPR > 0
  asm volatile("" ::: "v" BK_STR(BOURSE_AMD_FSM_TOP_VGPR));
#endif
  // MarketEnv mode (assets = M > 1): the lane owns a MARKET = books [b*M, b*M + M) with one RNG stream and one event
  // queue (market_env.rs:110-121, runner.rs:108-131); RandomMarketAgents::update is RandomAgents::update addressed to
  // the group's asset (random_agent.rs:204-247), so the state machine below is unchanged.
  const uint32_t M = a.assets;
  const uint32_t b = a.book_begin + blockIdx.x * 64 + lane;
  if (b >= a.book_end) return;
  uint32_t* st = a.state + (size_t)b * M * a.state_stride;
  uint32_t* bt = a.batch + (size_t)b * M * a.batch_stride;
#if BK_PB
  // the unit's row; group g + 1's loads are issued before group g's walk (the first ones before the state loads), so
  // only the first group's round trip is not hidden under a walk
  const Group* row = table + (size_t)b * a.n_groups;
  LaneGroup nxt{};
  if (a.n_groups) nxt = load_lane_group(row);
#endif

  RngLane rng;
  {
    const uint2 x0 = *reinterpret_cast<const uint2*>(st + H_S0_LO);
    const uint2 x1 = *reinterpret_cast<const uint2*>(st + H_S1_LO);
    rng.a0 = x0.x, rng.a1 = x0.y, rng.b0 = x1.x, rng.b1 = x1.y;
  }
  uint64_t live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint2 x = *reinterpret_cast<const uint2*>(st + H_LIVE0 + 2 * r);
    for (uint32_t as = 1; as < M; ++as) {  // slot = agent index in every book of the market: the masks are disjoint
      const uint2 y = *reinterpret_cast<const uint2*>(st + (size_t)as * a.state_stride + H_LIVE0 + 2 * r);
      x.x |= y.x;
      x.y |= y.y;
    }
    live[r] = mk64(x.x, x.y);
  }
  uint2* pv = reinterpret_cast<uint2*>(bt + BT_EV + 32 * R);

  // ---- loop 1: agents.update, group by group (declaration order).  Inside a group every lane runs a state
  // machine that performs exactly ONE next_u32() draw per iteration (a lane never waits for another lane's rejection
  // loop); the group's parameters are wave-uniform (SGPRs).  Lanes re-converge at each group boundary.
  // Select-style body (v_cndmask) with three short predicated blocks: list append, new-order store, next agent.
  const uint32_t five = RngLane::opaque5();
  uint32_t n = 0, n_ev = 0, gbase = 0;
  for (uint32_t g = 0; g < a.n_groups; ++g) {
    const Group G = a.groups[g];
    const uint32_t gend = gbase + G.n;
    gbase = gend;
#if BK_PB
    LaneGroup L{};  // (declared, then assigned: the PB kernel's code depends on this form)
    L = nxt;
    if (g + 1 < a.n_groups) nxt = load_lane_group(row + g + 1);
#endif
    if (G.n == 0) continue;
#if BK_PB
    // the lane's parameters are vector registers, made ready by the "v" fences below (a wait for vmcnt here)
    const uint32_t g_thr = L.a.y, g_tick_lo = L.a.z, g_vol_lo = L.b.y;
    uint32_t g_tick_size = L.tick_size;
    asm volatile("" : "+v"(g_tick_size));
    uint32_t v_trng = L.a.w, v_vrng = L.b.z, v_tzone = L.b.x, v_vzone = L.b.w;
#else
    // complete the scalar loads of the group's parameters HERE: a wait parked inside the loop would be
    // s_waitcnt lgkmcnt(0), which also waits for the iteration's own LDS writes (list append, ds_or) to drain
    asm volatile("" ::"s"(G.thr), "s"(G.tick_lo), "s"(G.tick_rng), "s"(G.tick_zone));
    asm volatile("" ::"s"(G.vol_lo), "s"(G.vol_rng), "s"(G.vol_zone), "s"(G.tick_size));
    const uint32_t g_thr = G.thr, g_tick_lo = G.tick_lo, g_vol_lo = G.vol_lo, g_tick_size = G.tick_size;
    uint32_t v_trng = G.tick_rng, v_vrng = G.vol_rng, v_tzone = G.tick_zone, v_vzone = G.vol_zone;
#endif
    // Every predicate of a draw is taken as a WAVE MASK first (v_cmp into an SGPR pair), then the generator's state
    // update runs (11 vector instructions that depend on none of them), and only then does the scalar unit combine the
    // masks: an SALU instruction that reads an SGPR a vector compare has JUST written stalls the wave ~16 clocks
    // (scripts/micro/lone_wave_latency.hip), and the straightforward form - `bool` predicates combined where they are
    // used - had five of those per draw (k_agents_fsm 161 -> 141 us per launch under load).  Same instructions, same
    // counts: the two fences only fix their order.
    // the group's ranges and zones as VECTOR registers for the loop: a select under an SGPR mask cannot also read an
    // SGPR source (one scalar operand per VOP3), so the compiler copied each of the four into a VGPR on every draw
    asm volatile("" : "+v"(v_trng), "+v"(v_vrng), "+v"(v_tzone), "+v"(v_vzone));
    // (BK_PB = 1: thr8 and tick_size are per lane - vector operands of the compare and of the multiply-add)
    const uint64_t thr8 = (uint64_t)g_thr << 8;
    // price = (tick_lo + val) * tick_size as one multiply-add: val * tick_size + tick_lo * tick_size (mod 2^32)
    uint64_t price0 = (uint64_t)(g_tick_lo * g_tick_size);
    asm volatile("" : "+v"(price0));  // (kept in a VGPR pair: the addend of the multiply-add below)
    // The group is walked in SEGMENTS that stay inside one 64-slot pool register, so that the live word of the agent
    // at hand is one register pair per segment, not a per-draw select over the pool's registers (lanes re-converge at
    // a segment's end as they do at a group's; the benchmark groups are 64-aligned: no extra boundary there).
    for (uint32_t sbeg = gend - G.n; sbeg < gend;) {
      const uint32_t send = gend < (sbeg | 63u) + 1u ? gend : (sbeg | 63u) + 1u;
      uint64_t w = live[0];
#pragma unroll
      for (int r = 1; r < R; ++r) w = ((sbeg >> 6) == (uint32_t)r) ? live[r] : w;
#if BK_FSM_HAND
      // the draw loop as ONE hand-written statement (fsm_asm.hpp); the C++ loop below is its specification, and the
      // kernel's second copy of this body (BK_FSM_HAND = 0, DevArgs::fsm_loop = 1) still runs it
      fsm_draw_asm(rng.a0, rng.a1, rng.b0, rng.b1, n, n_ev, v_trng, v_vrng, v_tzone, v_vzone,
                   (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)(list + lane),
                   __builtin_bitreverse64(w), pv, price0, thr8, g_tick_size, g_vol_lo, send);
#else
      uint32_t cur_side = 0, cur_price = 0;
      // The phase of every lane lives in four WAVE MASKS carried across the iterations in scalar registers (one-hot per
      // lane) and is advanced by scalar mask algebra at the end of the iteration - round 3 kept it in a vector register:
      // four compares to get the masks and four selects to write the next phase, every draw.  Bits of lanes that have
      // left the loop go stale, harmlessly: every predicate they are combined with is a ballot of the lanes still in it.
      uint64_t P_ACT = ~0ull, P_SIDE = 0, P_TICK = 0, P_VOL = 0;
      while (n < send) {
        const uint32_t x = rng.output(five);
        // range and zone of the phase at hand, from its masks (two selects each; no loop-carried copies)
        const uint32_t range = sel(P_SIDE, 2u, sel(P_TICK, v_trng, v_vrng));
        const uint32_t zone = sel(P_SIDE, 0x7FFFFFFFu, sel(P_TICK, v_tzone, v_vzone));
        const uint64_t m = (uint64_t)x * range;  // sample_single step of the current phase: accept iff lo <= zone
        const uint32_t val = (uint32_t)(m >> 32);
        // gen::<f32>() < activity_rate (:91-93): (x >> 8) < thr as ONE 64-bit compare x < thr << 8 (thr <= 2^24)
        uint64_t C_HIT = __builtin_amdgcn_ballot_w64((uint64_t)x < thr8);
        uint64_t C_ACC = __builtin_amdgcn_ballot_w64((uint32_t)m <= zone);
        uint64_t C_LIVE = __builtin_amdgcn_ballot_w64(((w >> (n & 63)) & 1ull) != 0);  // Active order held (:95-97)
        asm volatile("" : "+v"(rng.a0), "+v"(rng.a1), "+v"(rng.b0), "+v"(rng.b1)
                     : "s"(P_ACT), "s"(P_SIDE), "s"(P_TICK), "s"(P_VOL), "s"(C_HIT), "s"(C_ACC), "s"(C_LIVE));
        rng.advance();
        asm volatile("" : "+v"(rng.a0), "+v"(rng.a1), "+v"(rng.b0), "+v"(rng.b1), "+s"(P_ACT), "+s"(P_SIDE), "+s"(P_TICK),
                       "+s"(P_VOL), "+s"(C_HIT), "+s"(C_ACC), "+s"(C_LIVE));
        const uint64_t HIT = P_ACT & C_HIT, CANCEL = HIT & C_LIVE, TO_SIDE = HIT & ~C_LIVE;
        const uint64_t A_SIDE = C_ACC & P_SIDE, A_TICK = C_ACC & P_TICK, A_VOL = C_ACC & P_VOL;
        const uint64_t QUEUE = CANCEL | A_VOL, ADV = (P_ACT & ~C_HIT) | QUEUE;
        cur_side = sel(A_SIDE, val, cur_side);                                    // 0 = Ask, 1 = Bid ([Ask, Bid].choose, :99)
        {  // tick * tick_size (:100,:107)
          uint64_t pr, cy;
#if BK_PB
          asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(pr), "=s"(cy) : "v"(val), "v"(g_tick_size), "v"(price0));
#else
          asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(pr), "=s"(cy) : "v"(val), "s"(g_tick_size), "v"(price0));
#endif
          cur_price = sel(A_TICK, (uint32_t)pr, cur_price);
        }
        // the agent's event, queued once its kind is known (agent order): bit 15 = New, bit 14 = bid
        if (lane_bit(QUEUE)) list[n_ev * 64 + lane] = (uint16_t)sel(A_VOL, n | EV_NEW | (cur_side << 14), n);
        asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(n_ev) : "s"(QUEUE) : "vcc");  // n_ev += lane_bit(QUEUE)
        if (lane_bit(A_VOL)) pv[n] = make_uint2(cur_price, g_vol_lo + val);       // vol drawn last (:101): the order is complete
        // next phase; an agent that is done (inactive, cancelled or placed) hands over to the next one
        P_SIDE = TO_SIDE | (P_SIDE & ~C_ACC);
        P_TICK = A_SIDE | (P_TICK & ~C_ACC);
        P_VOL = A_TICK | (P_VOL & ~C_ACC);
        P_ACT = ADV;
        asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(n) : "s"(ADV) : "vcc");  // n += lane_bit(ADV)
      }
#endif
      sbeg = send;
    }
  }

  // ---- loop 2: transactions.shuffle(rng) (env.rs:121): for i in (1..n_ev).rev() { swap(i, gen_index(i + 1)) }
  // (rand SliceRandom::shuffle), again one draw per iteration per lane.
#if BK_FSM_HAND && (BOURSE_AMD_FSM_TAIL & 1)
  // ONE hand-written statement (fsm_asm.hpp); the C++ loop below is its specification
  fsm_shuffle_asm(rng.a0, rng.a1, rng.b0, rng.b1, n_ev,
                  (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)(list + lane));
#else
  {
    uint32_t i = n_ev > 1 ? n_ev - 1 : 0;
    uint32_t rg = i + 1;
    uint32_t zn = (rg << __builtin_clz(rg)) - 1u;
    while (i != 0) {
      const uint32_t x = rng.output(five);
      const uint64_t m = (uint64_t)x * rg;
      uint64_t ACC = __builtin_amdgcn_ballot_w64((uint32_t)m <= zn);  // (same ordering as in loop 1)
      asm volatile("" : "+v"(rng.a0), "+v"(rng.a1), "+v"(rng.b0), "+v"(rng.b1) : "s"(ACC));
      rng.advance();
      asm volatile("" : "+v"(rng.a0), "+v"(rng.a1), "+v"(rng.b0), "+v"(rng.b1), "+s"(ACC));
      if (lane_bit(ACC)) {
        const uint32_t j = (uint32_t)(m >> 32);
        const uint16_t ai = list[i * 64 + lane], aj = list[j * 64 + lane];
        list[i * 64 + lane] = aj;
        list[j * 64 + lane] = ai;
        --i;
        rg = i + 1;
        zn = (rg << __builtin_clz(rg)) - 1u;
      }
    }
  }
#endif

  // publish: RNG state back to the book header, the step batch for k_step_batch
  for (uint32_t as = 0; as < M; ++as) {  // every book of a market carries a copy of the market's RNG state
    *reinterpret_cast<uint2*>(st + (size_t)as * a.state_stride + H_S0_LO) = make_uint2(rng.a0, rng.a1);
    *reinterpret_cast<uint2*>(st + (size_t)as * a.state_stride + H_S1_LO) = make_uint2(rng.b0, rng.b1);
  }
  bt[BT_NEV] = n_ev;
#if BK_FSM_HAND && (BOURSE_AMD_FSM_TAIL & 2)
  // eight events per 16-byte store, the entries of the last group at or beyond n_ev written as 0 (fsm_asm.hpp).
  // NOTHING MAY FOLLOW THIS STATEMENT in the body: its global stores are neither waited for nor counted by the compiler,
  // so a load (or anything else the compiler waits for with a counted vmcnt) behind it could be released too early
  fsm_publish_asm(n_ev, (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)(list + lane), bt + BT_EV);
#else
  for (uint32_t k = 0; k < n_ev; k += 2) {
    const uint32_t lo = list[k * 64 + lane];
    const uint32_t hi = (k + 1 < n_ev) ? list[(k + 1) * 64 + lane] : 0u;
    bt[BT_EV + (k >> 1)] = lo | (hi << 16);
  }
#endif
