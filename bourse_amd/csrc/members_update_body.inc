// members_update_body.inc - one member's update(env, rng): the body of the loop over the members j of an AgentSet, ONE
// source text for k_update_members (members_ingress.hpp: the book's own walk) and k_update_market_members
// (market_ingress.hpp: the market's walk on the book of the member's asset), in the idiom of agents_fsm_body.inc.  As a
// function shared by the two kernels the same text moved k_update_members<1>'s loops beyond its committed profile.
//
// The including loop declares: g (list_cap, n_members, lists, lens, mstate), W, rng (= W.rng), row, id_start, mflags, j, lane,
// and of the book the member trades live[R], pid[R] (AGENT_HELD_NONE where nothing rests) and mid.  It defines
//   BK_MU_UNIT  the unit whose rows the member uses (the book, or the market)
//   BK_MU_TICK  the book's tick size (create_order's check)
//   BK_MU_TAG   what the member's events carry beside their kind (random_pass_end's tag)
// The RandomAgents branch leaves by `continue`.
    const MixedDesc D = sload_desc(row + j);
    uint32_t* list = g.lists + ((size_t)BK_MU_UNIT * g.n_members + j) * g.list_cap;
    if (D.type == 0) {
      // ---- RandomAgents::update (random_agent.rs:85-119): k_update_agents' pass over the member's held ids
      const uint32_t n_agents = min(D.n, g.list_cap);
      for (uint32_t base = 0; base < n_agents; base += 64) {
        const uint32_t n_here = min(64u, n_agents - base);
        const bool in = (uint32_t)lane < n_here;
        const uint32_t h = in ? list[base + lane] : AGENT_HELD_NONE;
        RandomPass S(W);
        // TraderId = the agent's index in its member
        for (uint32_t l = 0; l < n_here; ++l) random_agent<R>(W, S, D, pid, h, l, base + l);
        const uint32_t now = random_pass_end(W, S, h, BK_MU_TAG);
        if (in) list[base + lane] = now;
      }
      continue;
    }
    // ---- common::cancel_live_orders (common.rs:56-75): the Active entries in list order, one f32 draw each;
    // `draw > p_cancel` keeps the entry, otherwise its cancellation is queued and it leaves the list
    const uint32_t len0 = min(rfl(g.lens[(size_t)BK_MU_UNIT * g.n_members + j]), g.list_cap);
    uint32_t len = 0;
    for (uint32_t base = 0; base < len0; base += 64) {
      const bool in = base + (uint32_t)lane < len0;
      const uint32_t e = in ? list[base + lane] : AGENT_HELD_NONE;
      uint64_t actm = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (live[r] == 0) continue;
        for (uint32_t k = 0; k < 64; ++k) actm |= __ballot(e == rdl(pid[r], k));
      }
      // (an entry beyond the list, or a pool lane with nothing live, is AGENT_HELD_NONE on both sides)
      actm &= __ballot(in);
      const uint32_t ev0 = W.n_ev;
      uint64_t keepm = 0, canm = 0;
      for (uint64_t m = actm; m; m &= m - 1ull) {
        const uint64_t bit = m & (~m + 1ull);
        const uint32_t x = rng.next_u32();
        if ((int32_t)(x >> 8) > D.keep_thr) {
          keepm |= bit;
        } else if (W.n_ev < W.room) {  // env.cancel_order(id)
          canm |= bit;
          W.n_ev += 1;
        } else {
          W.flags |= FLAG_EVENT_OVERFLOW;
        }
      }
      const uint32_t rank_can = lane_rank(canm);
      const uint32_t rank_keep = lane_rank(keepm);
      if (lane_bit(canm)) W.q[W.q0 + ev0 + rank_can] = make_uint4(1u | BK_MU_TAG, e, 0u, 0u);
      if (lane_bit(keepm)) list[len + rank_keep] = e;  // (len + rank <= base + lane: behind every entry still to be read)
      len += (uint32_t)__builtin_popcountll(keepm);
    }
    // ---- the traders' loops (mixed_update_and_shuffle's, mixed_agents.hpp)
    const uint32_t trader0 = rfl(id_start[j]);
    NewBatch N;
    N.price = N.trader = 0;
    N.bidm = N.limm = 0;
    N.cnt = N.id0 = N.ev0 = 0;
    if (D.type == 1) {
      // ---- NoiseAgent::update (noise_agent.rs:127-176)
      for (uint32_t t = 0; t < D.n; ++t) {
        if ((rng.next_u32() >> 8) < D.thr_limit) {                 // gen::<f32>() < p_limit
          const bool buy = next_u64(rng) < 0x8000000000000000ull;  // gen_bool(0.5)
          const double dist = pm::fabs_(uni(pm::exp(D.mu + D.sigma * sample_standard_normal(rng))));
          const uint32_t price = rfl(buy ? round_price_down(mid - dist, D.tick_f) : round_price_up(mid + dist, D.tick_f));
          place_new(W, N, true, buy, price, trader0 + t, BK_MU_TICK, D.trade_vol, list, len, g.list_cap, lane, BK_MU_TAG);
        }
        if ((rng.next_u32() >> 8) < D.thr_market) {                // gen::<f32>() < p_market
          const bool buy = next_u64(rng) < 0x8000000000000000ull;
          place_new(W, N, false, buy, buy ? 0xFFFFFFFFu : 0u, trader0 + t, BK_MU_TICK, D.trade_vol, list, len, g.list_cap, lane, BK_MU_TAG);
        }
      }
    } else {
      // ---- MomentumAgent::update (momentum_agent.rs:146-208)
      uint64_t* ms = g.mstate + ((size_t)BK_MU_UNIT * g.n_members + j) * 2;
      double m = 0.0, p_market = 0.0;
      if ((mflags >> j) & 1u) {
        const double gm = uni(pm::from_bits(ms[0])), gl = uni(pm::from_bits(ms[1]));
        m = uni(gm * (1.0 - D.decay) + D.decay * (mid - gl));
        p_market = uni(D.demand * pm::tanh(D.scale * m) / D.n_f);
      }
      uint64_t thr_l, thr_m;
      {
        const double p_limit = D.order_ratio * p_market;
        thr_l = thr53(p_limit);
        thr_m = thr53(p_market);
        thr_l = mk64(rfl((uint32_t)thr_l), rfl((uint32_t)(thr_l >> 32)));
        thr_m = mk64(rfl((uint32_t)thr_m), rfl((uint32_t)(thr_m >> 32)));
      }
      const int sgn = (m > 0.0) ? 1 : ((m < 0.0) ? -1 : 0);
      for (uint32_t t = 0; t < D.n; ++t) {
        if ((next_u64(rng) >> 11) < thr_l) {  // gen::<f64>() < p_limit
          if (sgn != 0) {
            const double dist = pm::fabs_(uni(pm::exp(D.mu + D.sigma * sample_standard_normal(rng))));
            const uint32_t price =
                rfl(sgn > 0 ? round_price_down(mid - dist, D.tick_f) : round_price_up(mid + dist, D.tick_f));
            place_new(W, N, true, sgn > 0, price, trader0 + t, BK_MU_TICK, D.trade_vol, list, len, g.list_cap, lane, BK_MU_TAG);
          }
        }
        if ((next_u64(rng) >> 11) < thr_m) {  // gen::<f64>() < p_market
          if (sgn != 0)
            place_new(W, N, false, sgn > 0, sgn > 0 ? 0xFFFFFFFFu : 0u, trader0 + t, BK_MU_TICK, D.trade_vol, list, len,
                      g.list_cap, lane, BK_MU_TAG);
        }
      }
      if (lane == 0) {  // momentum, last_price, once per update
        ms[0] = pm::to_bits(m);
        ms[1] = pm::to_bits(mid);
      }
      mflags |= 1u << j;
    }
    flush_new(W, N, D.trade_vol, list, len, g.list_cap, lane, BK_MU_TAG);
    if (lane == 0) g.lens[(size_t)BK_MU_UNIT * g.n_members + j] = min(len, g.list_cap);
