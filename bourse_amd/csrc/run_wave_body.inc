// run_wave_body.inc - the body of k_run_wave (wave_agents.hpp), included by the uniform kernel with BK_PB = 0 and by its
// per-unit form with BK_PB = 1, whose decoder reads the book's row (table[book * n_groups + g]).  Included rather than
// called so that the uniform kernel compiles exactly as it did when this was its own source (see mixed_lanes_body.inc).
  constexpr int WPB = 8;                                       // books (waves) per workgroup
  constexpr int STAGE_DW = 128 * R > 256 ? 128 * R : 256;      // new orders {price, vol} by slot, then the level bins
  __shared__ uint4 tab[512];
  __shared__ uint32_t ring_s[WPB][WV_RING];
  __shared__ uint16_t evl_s[WPB][64 * R];
  __shared__ uint32_t pm_s[WPB][2 * R], sm_s[WPB][2 * R];
  __shared__ uint32_t stage_s[WPB][STAGE_DW];
  __shared__ uint16_t jarr_s[WPB][64 * R];
  __shared__ uint4 wmask_s[WPB][R <= 2 ? 128 : 1];  // the ring stays live across steps here: the masks get their own 2 KB
  const int lane = threadIdx.x & 63;
  const int wv = (int)rfl(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < 512; i += 512) tab[i] = wa.jt_block[i];
  __syncthreads();
  const uint32_t book = rfl(blockIdx.x * WPB + wv);
  if (book >= a.n_books) return;
  uint32_t* st = a.state + (size_t)book * a.state_stride;
  uint32_t* wc = wa.wcache + (size_t)book * WC_STRIDE;
  uint32_t* stage = stage_s[wv];

  Book<R> B;
  Rng rng;
  load_book<R>(B, rng, st, lane);
  WaveDecoder<R> D;
  D.tab = tab;
  D.ring = ring_s[wv];
  D.evl = evl_s[wv];
  D.pm = pm_s[wv];
  D.sm = sm_s[wv];
  D.pv = reinterpret_cast<uint2*>(stage);
  D.jarr = jarr_s[wv];
  D.wmask = wmask_s[wv];
  D.wcs = reinterpret_cast<uint4*>(wc + WC_HDR);
  D.lane = lane;
  D.load_cache(wc, (uint32_t)rng.s0, (uint32_t)(rng.s0 >> 32), (uint32_t)rng.s1, (uint32_t)(rng.s1 >> 32), wa.jt_lane);
  const uint32_t lim = 64u + (wa.lookahead < 1u ? 1u : (wa.lookahead > 64u ? 64u : wa.lookahead));
  uint64_t all[R];
#pragma unroll
  for (int r = 0; r < R; ++r) all[r] = ~0ull;
  uint32_t last_ntr = 0, last_nev = 0;

  for (uint32_t s = 0; s < n_steps; ++s) {
    // ---------------- agents.update(env, rng) + the shuffle of Env::step ----------------
    uint32_t livev = 0;  // lane w: bits [32 w, 32 w + 32) of the pool's live mask
#pragma unroll
    for (int r = 0; r < R; ++r) {
      livev = wrl((uint32_t)B.live[r], 2 * r, livev);
      livev = wrl((uint32_t)(B.live[r] >> 32), 2 * r + 1, livev);
    }
    if (lane < 2 * R) {
      D.pm[lane] = 0;
      D.sm[lane] = 0;
    }
    wave_sync();
#if BK_PB
    const Group* row = table + (size_t)book * a.n_groups;  // the book's row of the per-unit table
#else
    const Group* row = nullptr;
#endif
    const uint32_t n_ev = D.template agents<BK_PB>(a, lim, livev, 0u, R <= 2 ? mk64(rdl(livev, 0u), rdl(livev, 1u)) : 0ull,
                                                   R == 2 ? mk64(rdl(livev, 2u), rdl(livev, 3u)) : 0ull, row);
    D.shuffle(n_ev);
    // ---------------- the step's new orders into the pool (create_order ids: dense, agent order) -------------
    uint32_t ev[R];
    uint32_t base = B.next_id;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t pend = mk64(rfl(D.pm[2 * r]), rfl(D.pm[2 * r + 1]));
      const uint64_t side = mk64(rfl(D.sm[2 * r]), rfl(D.sm[2 * r + 1]));
      ev[r] = D.evl[r * 64 + lane];
      const uint2 pvv = D.pv[r * 64 + lane];
      B.price[r] = sel(pend, pvv.x, B.price[r]);
      B.vol[r] = sel(pend, pvv.y, B.vol[r]);
      const uint32_t rank = lane_rank(pend);
      B.id[r] = sel(pend, base + rank, B.id[r]);
      base += __builtin_popcountll(pend);
      B.bid[r] = (B.bid[r] & ~pend) | (side & pend);
      B.pend[r] = pend;  // handed to step_from_list, which clears it (the event words classify themselves: EV_NEW)
    }
    B.next_id = base;
    wave_sync();  // the staging area becomes the snapshot's level bins
    // ---------------- Env::step: events at t0 + k, clock, level-2 record, trades ----------------
    last_ntr = step_from_list<R, false, false, true>(B, a, book, lane, ev, n_ev, stage,
                                                     a.hist_cap ? (a.hist_slot0 + s) % a.hist_cap : 0u,
                                                     s + 1 == n_steps || a.hist_cap == 0, a.tick_div, all, last_nev);
    wave_sync();
  }
  uint32_t n0, n1, n2, n3;
  D.finish(wc, n0, n1, n2, n3);
  rng.s0 = mk64(n0, n1);
  rng.s1 = mk64(n2, n3);
  store_book<R>(B, rng, st, lane, first_step + n_steps, last_ntr, last_nev);
