// run_mixed_body.inc - the body of k_run_mixed (mixed_agents.hpp), included by the uniform kernel with BK_PB = 0
// and by its per-unit form with BK_PB = 1, which points ma.descs at the book's row of the table (member j: a scalar load
// as in the uniform kernel).  Included, not called, so that the uniform kernel compiles as it did (mixed_lanes_body.inc).
  __shared__ uint32_t lds[4][LDS_DW_PER_WAVE];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const uint32_t book = rfl(blockIdx.x * 4 + wv);
  if (book >= a.n_books) return;
  uint32_t* st = a.state + (size_t)book * a.state_stride;
#if BK_PB
  ma.descs = table + (size_t)book * ma.n_desc;
#endif

  Book<R> B;
  Rng rng;
  load_book<R>(B, rng, st, lane);
  MixedCtx<R> C;
  MixedState S;
  mixed_load_state(S, st, lane);
  mixed_load_ctx<R>(C, st, ma, lane);
  C.tick = a.tick_size;
  uint32_t last_ntr = 0, last_nev = 0;
  for (uint32_t s = 0; s < n_steps; ++s) {
    mixed_update_and_shuffle<R>(B, C, rng, ma, S, lane);
    last_ntr = step_from_list<R>(B, a, book, lane, C.ev, C.n_ev, lds[wv],
                                 a.hist_cap ? (a.hist_slot0 + s) % a.hist_cap : 0u, s + 1 == n_steps || a.hist_cap == 0,
                                 a.tick_div, B.pend, last_nev);
  }
  store_book<R>(B, rng, st, lane, first_step + n_steps, last_ntr, last_nev);
  mixed_store_state<R>(S, B, C, st, lane);
