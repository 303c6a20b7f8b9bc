// agents_mixed_body.inc - the body of k_agents_mixed (mixed_agents.hpp), included by the uniform kernel with BK_PB = 0
// and by its per-unit form with BK_PB = 1, which points ma.descs at the book's row of the table (member j: a scalar load
// as in the uniform kernel).  Included, not called, so that the uniform kernel compiles as it did (mixed_lanes_body.inc).
  const int lane = threadIdx.x & 63;
  const uint32_t book = rfl(a.book_begin + blockIdx.x * 4 + (threadIdx.x >> 6));
  if (book >= a.book_end) return;
  uint32_t* st = a.state + (size_t)book * a.state_stride;
  uint32_t* bt = a.batch + (size_t)book * a.batch_stride;
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
  mixed_update_and_shuffle<R>(B, C, rng, ma, S, lane);
  // the step counter / last-step figures are k_step_batch's to write: keep the header's values
  const uint32_t hdr = st[lane];
  store_book<R>(B, rng, st, lane, mk64(rdl(hdr, H_STEPS_LO), rdl(hdr, H_STEPS_HI)), rdl(hdr, H_LAST_NTRADES),
                rdl(hdr, H_LAST_NEVENTS));
  mixed_store_state<R>(S, B, C, st, lane);
  if (lane == 0) bt[BT_NEV] = C.n_ev;
#pragma unroll
  for (int r = 0; r < R; ++r) reinterpret_cast<uint16_t*>(bt + BT_EV)[r * 64 + lane] = (uint16_t)C.ev[r];
