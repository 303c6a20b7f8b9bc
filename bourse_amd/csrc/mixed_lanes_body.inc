// mixed_lanes_body.inc - the body of k_agents_mixed_lanes (mixed_agents.hpp), included by the uniform kernel with
// BK_PB = 0 and by its per-unit form (bk_set_agents_per_book) with BK_PB = 1.  The text is shared so that the two
// cannot drift apart, and included rather than called so that the uniform kernel compiles exactly as it did when this was
// its own source (an inlined shared body changes the compiled code: the callee is simplified before it is inlined).
// BK_PB = 1: the member's parameters are per lane (the lane's book or market u = b: table[u * n_desc + j]), loaded
// for the fields its kind uses (lane_desc), and the deferred-price queue rounds each entry with its own book's tick.
  // dynamic LDS (up to ~82 KB at R = 8; MI355X allows 160 KB per workgroup), see mixed_lanes_lds_bytes():
  //   event list of lane l: list[k * 64 + l] (u16) | live / listed masks of the open book, word w of lane l at
  //   [w * 64 + l] | per-asset allocation cursors (MKT) | ziggurat tables.  Everything a lane looks up per order lives
  //   here: with one wave per SIMD every global round trip is exposed latency.
  extern __shared__ uint32_t smem[];
  uint16_t* list = reinterpret_cast<uint16_t*>(smem);
  uint32_t* lds_live = smem + 32 * R * 64;
  uint32_t* lds_inl = lds_live + 2 * R * 64;
  uint32_t* cur_w = lds_inl + 2 * R * 64;
  uint32_t* cur_c = cur_w + (MKT ? MAX_ASSETS * 64 : 64);
  double* zx = reinterpret_cast<double*>(cur_c + (MKT ? MAX_ASSETS * 64 : 64));
  double* zf = zx + 257;
  // Deferred limit prices (not MKT): a member's turn draws and decides for the 64 books in lockstep, but only the few
  // lanes whose agent places an order need exp() and the tick rounding - 150 f64 instructions at 5-9 % lane
  // utilisation, 60 % of this kernel's vector work (profiles/r02/pmc_c5m.json).  Those lanes create the order without a
  // price and queue {exp argument, mid, book lane, slot}; whenever 64 entries are waiting, ALL lanes take one each.
  // Same arithmetic on the same operands, so the same bits.  Orders that might reach the u32::MAX clamp (the one case
  // whose outcome - Err, nothing created - changes what is drawn next) keep the in-line path.
  double* q_arg = zf + 257;
  double* q_mid = q_arg + MLQ_CAP;
  uint32_t* q_info = reinterpret_cast<uint32_t*>(q_mid + MLQ_CAP);
#if BK_PB
  // PB: a queued price is rounded with its own book's tick - the member's tick_f of each lane, written at the member's start
  double* q_tick = reinterpret_cast<double*>(q_info + MLQ_CAP);
#endif
  const int lane = threadIdx.x;
  for (int i = lane; i < 257; i += 64) {
    zx[i] = ZIG_NORM_X[i];
    zf[i] = ZIG_NORM_F[i];
  }
  __syncthreads();
  const uint32_t b = a.book_begin + blockIdx.x * 64 + lane;  // book, or market when MKT
  if (b >= a.book_end) return;
  const uint32_t M = MKT ? a.assets : 1u;
  uint32_t* st0 = a.state + (size_t)b * M * a.state_stride;
  uint32_t* bt = a.batch + (size_t)b * M * a.batch_stride;
  const size_t NB = ml.n_books, NU = ml.n_units;
  const uint64_t act = __builtin_amdgcn_ballot_w64(true);  // the lanes with a book (all 64 but in the last workgroup)
  const uint32_t n_act = __builtin_popcountll(act);
  const uint32_t my_rank = lane_rank(act);

  LaneRng rng;
  {
    const uint2 x0 = *reinterpret_cast<const uint2*>(st0 + H_S0_LO);
    const uint2 x1 = *reinterpret_cast<const uint2*>(st0 + H_S1_LO);
    rng.s0 = mk64(x0.x, x0.y);
    rng.s1 = mk64(x1.x, x1.y);
  }
  uint32_t n_ev = 0;
  // the book the current member trades on
  uint32_t* st = st0;
  uint32_t bk = b * M, asset = 0, n_fixed = MKT ? ma.n_fixed_a[0] : ma.n_fixed;
  uint32_t next_id = 0, new_flags = 0;
  // slot allocation cursor: word `wcur` of the occupancy (live | listed | allocated this step), lowest free bit first
  uint32_t wcur = 0, cw = 0xFFFFFFFFu;
  // stage the open book's live masks (one 64-byte line of its header) and listed masks in LDS / write the latter back
  auto stage_masks = [&]() {
#pragma unroll
    for (int q = 0; q < (2 * R) / 4; ++q) {
      const uint4 v = *reinterpret_cast<const uint4*>(st + H_LIVE0 + 4 * q);
      lds_live[(4 * q + 0) * 64 + lane] = v.x;
      lds_live[(4 * q + 1) * 64 + lane] = v.y;
      lds_live[(4 * q + 2) * 64 + lane] = v.z;
      lds_live[(4 * q + 3) * 64 + lane] = v.w;
    }
    if (R == 1) {
      lds_live[lane] = st[H_LIVE0];
      lds_live[64 + lane] = st[H_LIVE0 + 1];
    }
#pragma unroll
    for (int w = 0; w < 2 * R; ++w) lds_inl[w * 64 + lane] = ml.inl[(size_t)w * NB + bk];
  };
  auto unstage_masks = [&]() {
#pragma unroll
    for (int w = 0; w < 2 * R; ++w) ml.inl[(size_t)w * NB + bk] = lds_inl[w * 64 + lane];
  };
  auto load_word = [&](uint32_t w) -> uint32_t {
    uint32_t v = lds_live[w * 64 + lane] | lds_inl[w * 64 + lane];
    if (n_fixed > 32u * w) v |= (n_fixed - 32u * w >= 32u) ? 0xFFFFFFFFu : ((1u << (n_fixed - 32u * w)) - 1u);
    return v;
  };
  if (MKT) {
    for (uint32_t as = 0; as < M; ++as) cur_w[as * 64 + lane] = 0xFFFFFFFFu;  // not opened yet
  } else {
    stage_masks();
    wcur = n_fixed >> 5;
    if (wcur < 2u * R) cw = load_word(wcur);
    next_id = st[H_NEXT_ID];
  }
  auto open_book = [&](uint32_t as) {  // MKT: switch to the member's asset
    asset = as;
    st = st0 + (size_t)as * a.state_stride;
    bk = b * M + as;
    n_fixed = ma.n_fixed_a[as];
    next_id = st[H_NEXT_ID];
    new_flags = 0;
    stage_masks();
    wcur = cur_w[as * 64 + lane];
    cw = cur_c[as * 64 + lane];
    if (wcur == 0xFFFFFFFFu) {
      wcur = n_fixed >> 5;
      cw = wcur < 2u * R ? load_word(wcur) : 0xFFFFFFFFu;
    }
  };
  auto close_book = [&]() {
    unstage_masks();
    st[H_NEXT_ID] = next_id;
    if (new_flags) st[H_FLAGS] |= new_flags;
    cur_w[asset * 64 + lane] = wcur;
    cur_c[asset * 64 + lane] = cw;
  };
  auto pool_ptr = [&](uint32_t slot, int field) -> uint32_t* {
    return st + HDR_DW + (slot >> 6) * (POOL_FIELDS * 64) + field * 64 + (slot & 63u);
  };
  // The step's event list holds 64 * R entries per unit.  One book can never queue more (every event refers to its own
  // pool slot); a MARKET's joint queue can, when its books together keep more than one pool's worth of orders in play:
  // the event is then dropped and the book flagged (BK_FLAG_EVENT_OVERFLOW) - never written past the list.
  auto event_room = [&]() -> bool {
    if (n_ev < 64u * R) return true;
    new_flags |= FLAG_EVENT_OVERFLOW;
    return false;
  };
  auto push_event = [&](uint32_t slot) {
    list[n_ev * 64 + lane] = (uint16_t)(slot | (asset << 12));
    n_ev += 1;
  };
  // Env::place_order from a member: id + New event; returns the slot (or 0xFFFF when the pool is full: flagged)
  auto create = [&](bool is_bid, uint32_t price, uint32_t vol, uint32_t tag, bool deferred = false) -> uint32_t {
    // create_order's tick check (orderbook.rs:367-382): the reference `.unwrap()`s the Err, i.e. panics — flagged, and
    // like an Err nothing is created (see mixed_create).  Market orders (tag 0 here) carry no price.  (A deferred price
    // is a tick multiple below the clamp by construction.)
    if (!deferred && tag != 0 && price % (MKT ? a.asset_tick[asset] : a.tick_size) != 0) {
      new_flags |= FLAG_PRICE_TICK;
      return 0xFFFFu;
    }
    if (!event_room()) return 0xFFFFu;
    const uint32_t id = next_id;
    next_id += 1;  // create_order consumes the id (orderbook.rs:363)
    while (cw == 0xFFFFFFFFu && wcur < 2u * R) {
      wcur += 1;
      if (wcur < 2u * R) cw = load_word(wcur);
    }
    if (wcur >= 2u * R) {
      new_flags |= FLAG_POOL_OVERFLOW;  // reported, never silent: the order (and its event) is dropped
      return 0xFFFFu;
    }
    const uint32_t bit = __builtin_ctz(~cw);
    cw |= 1u << bit;
    const uint32_t slot = wcur * 32u + bit;
    if (!deferred) *pool_ptr(slot, 0) = price;
    *pool_ptr(slot, 1) = vol;
    *pool_ptr(slot, 2) = id;
    *pool_ptr(slot, 4) = 4u | (is_bid ? 2u : 0u) | (tag << 8);  // pending New
    push_event(slot);
    return slot;
  };
  // ---- deferred limit prices (see q_arg above)
  const uint32_t wave_b0 = a.book_begin + blockIdx.x * 64;
  // limit order at mid -/+ exp(arg): in line when a sell might reach the clamp (or in a market), otherwise created
  // without its price and handed to `queue_turn` below
  uint32_t qc = 0;  // entries waiting (wave-uniform)
  bool pend_q = false;
  double pend_arg = 0.0;
  uint32_t pend_info = 0;
  auto place_limit = [&](bool buy, double arg, double mid, double lnslack, const MixedDesc& D, uint32_t tag) -> uint32_t {
    if (MKT || !(buy || arg < lnslack)) {
      const double dist = pm::fabs_(pm::exp(arg));
      const uint32_t price = buy ? round_price_down(mid - dist, D.tick_f) : round_price_up(mid + dist, D.tick_f);
      return create(buy, price, D.trade_vol, tag);
    }
    const uint32_t slot = create(buy, 0u, D.trade_vol, tag, true);
    if (slot != 0xFFFFu) {
      pend_q = true;
      pend_arg = arg;
      pend_info = (uint32_t)lane | (slot << 6) | (buy ? 0x8000u : 0u);
    }
    return slot;
  };
  // all lanes, 64 (or, with `all`, whatever is left) queued orders: one each
  auto drain = [&](bool all, double tick_f) {
    if (MKT) return;
    while (qc >= (all ? 1u : 64u)) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint32_t take = qc < 64u ? qc : 64u, base = qc - take;
      for (uint32_t e = my_rank; e < take; e += n_act) {
        const double arg = q_arg[base + e], mid_e = q_mid[base + e];
        const uint32_t info = q_info[base + e], slot = (info >> 6) & 0x1FFu;
        const double dist = pm::fabs_(pm::exp(arg));
#if BK_PB
        const double tick_e = q_tick[info & 63u];
        (void)tick_f;
        const uint32_t price = (info & 0x8000u) ? round_price_down(mid_e - dist, tick_e) : round_price_up(mid_e + dist, tick_e);
#else
        const uint32_t price = (info & 0x8000u) ? round_price_down(mid_e - dist, tick_f) : round_price_up(mid_e + dist, tick_f);
#endif
        uint32_t* sb = a.state + (size_t)(wave_b0 + (info & 63u)) * a.state_stride;
        sb[HDR_DW + (slot >> 6) * (POOL_FIELDS * 64) + (slot & 63u)] = price;
      }
      qc = base;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };
  // at the end of an agent's turn, where the lanes are together again: the orders placed in it join the queue
  auto queue_turn = [&](double mid, double tick_f) {
    if (MKT) return;
    const uint64_t w = __builtin_amdgcn_ballot_w64(pend_q);
    if (w == 0) return;
    if (pend_q) {
      const uint32_t q = qc + lane_rank(w);
      q_arg[q] = pend_arg;
      q_mid[q] = mid;
      q_info[q] = pend_info;
    }
    pend_q = false;
    qc += __builtin_popcountll(w);
    drain(false, tick_f);
  };
  // a sell at mid + exp(arg), rounded UP to the tick, stays below the u32::MAX clamp when arg < lnslack
  auto clamp_bound = [&](double mid, double tick_f) -> double {
    const double slack = 4294967295.0 - mid - 2.0 * tick_f - 1.0;
    return slack > 1.0 ? pm::log(slack) - 1e-9 : -1e300;
  };

  for (uint32_t j = 0; j < ma.n_desc; ++j) {  // members in declaration order (crates/macros/src/lib.rs:57-73)
#if BK_PB
    // the shared fields (type, n, slot_base, n_f) of unit 0's row, the rest from this lane's unit's row
    MixedDesc D = ma.descs[j];
    lane_desc(D, table + ((size_t)b * ma.n_desc + j));
    if (!MKT) q_tick[lane] = D.tick_f;  // (the previous member's queue is empty: drain(true) at its end)
#else
    const MixedDesc D = ma.descs[j];
#endif
    if (MKT) open_book(ma.asset[j]);
    // OrderBook::mid_price (orderbook.rs:272-276): the touches of the book's last level-2 record (updates only queue
    // events, so the book is still the one that record describes)
    double mid;
    {
      const uint32_t* l2 = a.l2_last + (size_t)bk * a.l2_width;
      const uint32_t bid = l2[1], ask = l2[2];
      mid = static_cast<double>(bid) + 0.5 * static_cast<double>(ask - bid);
    }
    if (D.type == 0) {
      // ---- RandomAgents::update (random_agent.rs:85-119), fixed slots [slot_base, slot_base + n)
      uint32_t lw = 0;
      for (uint32_t i = 0; i < D.n; ++i) {
        const uint32_t n = D.slot_base + i;
        if (i == 0 || (n & 31u) == 0) lw = lds_live[(n >> 5) * 64 + lane];
        const uint32_t x = rng.next_u32();
        if ((x >> 8) < D.thr && event_room()) {
          push_event(n);
          if (!((lw >> (n & 31u)) & 1u)) {
            const uint32_t side = rng.below(2u, 0x7FFFFFFFu);
            const uint32_t tick = D.tick_lo + rng.below(D.tick_rng, D.tick_zone);
            const uint32_t vol = D.vol_lo + rng.below(D.vol_rng, D.vol_zone);
            *pool_ptr(n, 0) = tick * D.tick_size;
            *pool_ptr(n, 1) = vol;
            *pool_ptr(n, 2) = next_id;
            *pool_ptr(n, 4) = 4u | (side ? 2u : 0u);
            next_id += 1;
          }
        }
      }
      if (MKT) close_book();
      continue;
    }
    // ---- common::cancel_live_orders (common.rs:56-75): Active orders of the list in order, one f32 draw each
    const uint32_t tag = j + 1;
    uint16_t* my = ml.list + (size_t)j * ml.cap * NU + b;
    uint32_t len = ml.len[(size_t)j * NU + b], keep = 0;
    {
      // entries are fetched eight at a time BEFORE any of them is processed: the list is compacted in place (writes
      // never pass the read position), and a load issued after a store to the same array would wait for it
      uint32_t lw = 0, lwi = 0xFFFFFFFFu;
      for (uint32_t i0 = 0; i0 < len; i0 += 8) {
        uint32_t ent[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) ent[q] = (i0 + q < len) ? my[(size_t)(i0 + q) * NU] : 0xFFFFu;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const uint32_t slot = ent[q];
          if (slot == 0xFFFFu) continue;
          if ((slot >> 5) != lwi) {
            lwi = slot >> 5;
            lw = lds_live[lwi * 64 + lane];
          }
          if (!((lw >> (slot & 31u)) & 1u)) {  // filled or cancelled meanwhile: forget it, the slot becomes allocatable
            atomicAnd(&lds_inl[(slot >> 5) * 64 + lane], ~(1u << (slot & 31u)));  // ds_and, nothing to wait for
            continue;
          }
          const uint32_t x = rng.next_u32();
          if ((int32_t)(x >> 8) > D.keep_thr) {  // gen::<f32>() > p_cancel: kept
            my[(size_t)keep * NU] = (uint16_t)slot;
            keep += 1;
          } else if (event_room()) {  // env.cancel_order(id); stays live (and unallocatable) until the event is processed
            push_event(slot);
            atomicAnd(&lds_inl[(slot >> 5) * 64 + lane], ~(1u << (slot & 31u)));  // ds_and, nothing to wait for
          } else {  // no room for the cancellation (flagged): the order stays the member's
            my[(size_t)keep * NU] = (uint16_t)slot;
            keep += 1;
          }
        }
      }
    }
    auto remember = [&](uint32_t slot) {  // live_orders.push(order_id)
      if (slot == 0xFFFFu) return;
      my[(size_t)keep * NU] = (uint16_t)slot;
      keep += 1;
      atomicOr(&lds_inl[(slot >> 5) * 64 + lane], 1u << (slot & 31u));
    };
    const double lnslack = MKT ? 0.0 : clamp_bound(mid, D.tick_f);
    if (D.type == 1) {
      // ---- NoiseAgent::update (noise_agent.rs:127-176)
      for (uint32_t t = 0; t < D.n; ++t) {
        if ((rng.next_u32() >> 8) < D.thr_limit) {                   // gen::<f32>() < p_limit
          const bool buy = rng.next_u64() < 0x8000000000000000ull;   // gen_bool(0.5)
          remember(place_limit(buy, D.mu + D.sigma * rng.std_normal(zx, zf), mid, lnslack, D, tag));
        }
        if ((rng.next_u32() >> 8) < D.thr_market) {                  // gen::<f32>() < p_market
          const bool buy = rng.next_u64() < 0x8000000000000000ull;
          create(buy, buy ? 0xFFFFFFFFu : 0u, D.trade_vol, 0u);
        }
        queue_turn(mid, D.tick_f);
      }
      drain(true, D.tick_f);
    } else {
      // ---- MomentumAgent::update (momentum_agent.rs:146-208)
      double m = 0.0, p_market = 0.0;
      const uint32_t gflags = st[H_GFLAGS];
      if ((gflags >> j) & 1u) {
        const double gm = pm::from_bits(mk64(st[H_GST + 4 * j], st[H_GST + 4 * j + 1]));
        const double gl = pm::from_bits(mk64(st[H_GST + 4 * j + 2], st[H_GST + 4 * j + 3]));
        m = gm * (1.0 - D.decay) + D.decay * (mid - gl);
        p_market = D.demand * pm::tanh(D.scale * m) / D.n_f;
      }
      const uint64_t thr_l = thr53(D.order_ratio * p_market), thr_m = thr53(p_market);
      const int sgn = (m > 0.0) ? 1 : ((m < 0.0) ? -1 : 0);
      for (uint32_t t = 0; t < D.n; ++t) {
        if ((rng.next_u64() >> 11) < thr_l) {  // gen::<f64>() < p_limit
          if (sgn != 0) remember(place_limit(sgn > 0, D.mu + D.sigma * rng.std_normal(zx, zf), mid, lnslack, D, tag));
        }
        if ((rng.next_u64() >> 11) < thr_m) {  // gen::<f64>() < p_market
          if (sgn != 0) create(sgn > 0, sgn > 0 ? 0xFFFFFFFFu : 0u, D.trade_vol, 0u);
        }
        queue_turn(mid, D.tick_f);
      }
      drain(true, D.tick_f);
      const uint64_t mb = pm::to_bits(m), lb = pm::to_bits(mid);
      st[H_GST + 4 * j] = (uint32_t)mb;
      st[H_GST + 4 * j + 1] = (uint32_t)(mb >> 32);
      st[H_GST + 4 * j + 2] = (uint32_t)lb;
      st[H_GST + 4 * j + 3] = (uint32_t)(lb >> 32);
      st[H_GFLAGS] = gflags | (1u << j);
    }
    ml.len[(size_t)j * NU + b] = keep;
    if (MKT) close_book();
  }

  // ---- transactions.shuffle(rng) (env.rs:121)
  {
    uint32_t i = n_ev > 1 ? n_ev - 1 : 0;
    while (i != 0) {
      const uint32_t rg = i + 1;
      const uint32_t jx = rng.below(rg, (rg << __builtin_clz(rg)) - 1u);
      const uint16_t ai = list[i * 64 + lane], aj = list[jx * 64 + lane];
      list[i * 64 + lane] = aj;
      list[jx * 64 + lane] = ai;
      --i;
    }
  }
  for (uint32_t as = 0; as < M; ++as) {  // every book of a market carries a copy of the market's RNG state
    uint32_t* h = st0 + (size_t)as * a.state_stride;
    *reinterpret_cast<uint2*>(h + H_S0_LO) = make_uint2((uint32_t)rng.s0, (uint32_t)(rng.s0 >> 32));
    *reinterpret_cast<uint2*>(h + H_S1_LO) = make_uint2((uint32_t)rng.s1, (uint32_t)(rng.s1 >> 32));
  }
  if (!MKT) {
    unstage_masks();
    st[H_NEXT_ID] = next_id;
    if (new_flags) st[H_FLAGS] |= new_flags;
  }
  bt[BT_NEV] = n_ev;
  for (uint32_t k = 0; k < n_ev; k += 2) {
    const uint32_t lo = list[k * 64 + lane];
    const uint32_t hi = (k + 1 < n_ev) ? list[(k + 1) * 64 + lane] : 0u;
    bt[BT_EV + (k >> 1)] = lo | (hi << 16);
  }
