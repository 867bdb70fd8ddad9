// The world pool's host side: the generation launches, the batch scheduler and the adoption of the caller's stream.
// Included by crafter_hip.hip only, once, behind handle.hpp.
#pragma once

// The three kernels of generation batch `seq` over request segment `seg`, for the plan's GEO
template <int GEO>
static void launch_generation(crafter_handle* h, hipStream_t side, dim3 gs, dim3 gc, int seg, uint32_t seq, int prio) {
  hipLaunchKernelGGL(crafter_gen_seed_kernel<GEO>, gs, dim3(kGenSeedThreads), kGenSeedLds, side, h->cfg, h->tb, h->st, seg, prio, (const LevelTable*)h->levels);
  hipLaunchKernelGGL(crafter_gen_classify_kernel<GEO>, gc, dim3(kGenClassifyThreads), gen_classify_lds_bytes(h->cfg), side, h->cfg, h->tb, h->st, seg, h->gen_classify_prio);
  hipLaunchKernelGGL(crafter_gen_resolve_kernel<GEO>, gs, dim3(kGenResolveThreads), h->gen_resolve_lds_bytes, side, h->cfg, h->tb,
                     h->st, seg, seq, prio);
}
#ifdef CRAFTER_PROBES
template <int GEO>
static void launch_generation_stamp(crafter_handle* h, hipStream_t side, int seg, uint32_t seq) {
  hipLaunchKernelGGL(crafter_gen_stamp_kernel<GEO>, dim3(64), dim3(kStepThreads), 0, side, h->cfg, h->tb, h->st, seg, seq);
}
#endif

// World-pool scheduler, once per crafter_step (after the step's kernels are enqueued).  Any HIP failure here
// disables the pool for good (pool_failed): worlds of batches <= safe_seq stay valid, nothing newer is ever
// trusted, finished envs regenerate inline (gen_parity = -1 in StepCtl) -- slower, never wrong.
static void pool_fail(crafter_handle* h, const char* what, hipError_t e) {
  h->pool_failed = true;
  h->pool_err = std::string("world pool disabled (") + what + ": " + hipGetErrorString(e) + "); finished envs regenerate inline";
}

// Trust in batches polled_seq + 1 .. safe_seq rests on hipStreamWaitEvent calls enqueued on ONE stream (safe_stream).  The
// header only asks the caller to serialise the calls on a handle, not to keep to one stream: a call that arrives on
// another stream gets the same waits before any of its kernels is enqueued (a reset() under
// torch.cuda.stream(s) followed by step() on another stream trusted batches that stream had never waited for).
static void pool_adopt_stream(crafter_handle* h, hipStream_t stream) {
  if (!pool_live(h)) return;
  if (h->have_safe_stream && h->safe_stream == stream) return;
  if (h->have_safe_stream)
    for (uint32_t s = (h->safe_seq > h->polled_seq + kGenRing ? h->safe_seq - kGenRing : h->polled_seq) + 1; s <= h->safe_seq; s++) {
      // (an event slot older than the ring has been recorded again by a later batch of the same side stream: waiting for
      // that one is waiting for more)
      hipError_t ew = hipStreamWaitEvent(stream, h->ev_gen[s % kGenRing], 0);
      if (ew != hipSuccess) {
        pool_fail(h, "hipStreamWaitEvent(new launch stream)", ew);
        h->safe_seq = h->polled_seq;
        break;
      }
    }
  h->safe_stream = stream;
  h->have_safe_stream = true;
}

// Every entry point that enqueues kernels takes the caller's stream.  The header promises that a caller who changes streams
// between calls need not order them himself: the new stream waits for whatever the handle still has in flight on the
// previous one (an event recorded there) -- whether or not the world pool runs (crafter_reset on stream A followed
// by crafter_step on stream B raced the reset kernel) -- and then for the pool batches the old stream had been ordered behind.
static int adopt_stream(crafter_handle* h, hipStream_t stream) {
  if (h->have_last_stream && h->last_stream != stream) {
    if (!h->ev_switch) {
      hipError_t ec = hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming);
      if (ec != hipSuccess) return hip_fail(h, "stream change: hipEventCreate", ec);
    }
    hipError_t e = hipEventRecord(h->ev_switch, h->last_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, h->ev_switch, 0);
    if (e != hipSuccess) {
      // The previous stream may be gone (a C caller may destroy a stream once its work is done -- ADVICE r5: the failed record
      // used to leave last_stream pointing at it, and every later call failed the same way).  Everything the handle enqueued
      // there is then ordered the blunt way, once, and the handle moves on to the new stream.
      (void)hipGetLastError();
      hipError_t es = hipDeviceSynchronize();
      if (es != hipSuccess) return hip_fail(h, "stream change: ordering the new stream behind the previous one", es);
    }
  }
  h->last_stream = stream;
  h->have_last_stream = true;
  pool_adopt_stream(h, stream);
  return 0;
}

// main_recorded: ev_main already marks the point of the launch stream the batch has to wait for (crafter_step_n: it is the
// stop event of the stretch's last kernel -- that kernel's own completion signal instead of a marker packet of its own
// behind it: every packet between two dependent kernels costs the launch stream 4-5 us here, profiles/r5_rollout_gaps.txt)
static void pool_schedule(crafter_handle* h, hipStream_t main, int steps = 1, bool main_recorded = false, bool behind_rollout = false) {
  // 1. trust: batches complete in launch order per stream but the two streams interleave, so poll in sequence order
  while (h->polled_seq < h->batches) {
    hipError_t q = hipEventQuery(h->ev_gen[(h->polled_seq + 1) % kGenRing]);
    if (q == hipSuccess) {
      h->polled_seq++;
      if (h->safe_seq < h->polled_seq) h->safe_seq = h->polled_seq;
    } else if (q == hipErrorNotReady) {
      break;
    } else {
      return pool_fail(h, "hipEventQuery", q);
    }
  }
  h->steps_since_gen += steps;
  if (h->steps_since_gen < h->gen_period) return;
  // 2. back-pressure: order the launch stream behind batch seq - kGenLag (no host wait).  This also covers the reuse
  //    of queue segment / event slot seq % kGenRing, last used by batch seq - kGenRing + 1 <= seq - kGenLag.
  uint32_t seq = h->batches + 1;
  if (seq > (uint32_t)h->gen_lag + 1 && h->safe_seq < seq - h->gen_lag) {
    uint32_t t = seq - h->gen_lag;
    hipError_t ew = hipStreamWaitEvent(main, h->ev_gen[t % kGenRing], 0);
    if (ew != hipSuccess) return pool_fail(h, "hipStreamWaitEvent(launch stream)", ew);
    h->safe_seq = t;   // steps enqueued from now on run after batch t
  }
  // 3. launch batch `seq` over the segment that has been collecting
  hipStream_t side = h->side[seq % kGenStreams];
  hipError_t e = main_recorded ? hipSuccess : hipEventRecord(h->ev_main, main);
  if (e != hipSuccess) return pool_fail(h, "hipEventRecord(launch stream)", e);
  e = hipStreamWaitEvent(side, h->ev_main, 0);
  if (e != hipSuccess) return pool_fail(h, "hipStreamWaitEvent(generation stream)", e);
  // (Consecutive batches run side by side on the two streams.  They never write the same pool entry: a request whose
  // entry still has an older generation on its way is put off on the device, request_generation / PoolHdr.pending.)
  int seg = h->gen_parity;
  int n = h->cfg.num_envs;
  // Wave priority of the batch's two one-wave-per-world kernels (seeding, ordered draws: a few hundred waves whose serial
  // chain is the batch's latency; the classification in between stays at 0).  Behind a rollout stretch 2: the launch
  // stream of an open loop runs far ahead of the host's polling, every stretch waits for batch seq - 3 on the device, and
  // on every second stretch that wait was a real one (profiles/r5_rollout_gaps.txt): open loop 74.5-74.9 -> 75.6-75.9 M.
  // Behind a closed-loop step 1 (round 6; 0 until then: priority 2 costs the 64x64 loop 0.5 %, 64.7 -> 64.4 M): the ordered draws of
  // a 256x256 world are a 7 ms chain, and BASELINE configs[3] -- bound by its generator -- runs at 15.05-15.12 M env-steps/s with it
  // against 14.25-14.59 M (profiles/r6_cfg4_prio.txt; 2 and 3: the same); the 64x64 loop's 20-step window gains 1.5 %, its
  // steady state loses 0.2 % (profiles/r6_headline_prio.txt).
  const int prio = h->gen_serial_prio >= 0 ? h->gen_serial_prio : (behind_rollout ? 2 : 1);
  const int cgrid = behind_rollout ? h->classify_grid : h->classify_grid_step;
  dim3 gs(n < kGenSerialGrid ? n : kGenSerialGrid), gc((long long)n * gen_classify_parts(h->cfg) < cgrid ? n * gen_classify_parts(h->cfg) : cgrid);
#ifdef CRAFTER_PROBES
  if (h->probe_free_gen) {   // timing probe: see crafter_gen_stamp_kernel
    if (h->probe_free_gen == 2) {   // ... behind workgroups that occupy what the three kernels occupy, for as long (profiles/r5_kernel_stats.csv)
      const int worlds = h->probe_worlds > 0 ? h->probe_worlds : 390;
      int ws = worlds < (int)gs.x ? worlds : (int)gs.x, wc = worlds * gen_classify_parts(h->cfg) < (int)gc.x ? worlds * gen_classify_parts(h->cfg) : (int)gc.x;
      const int l0 = h->probe_lds[0] >= 0 ? h->probe_lds[0] : kGenSeedLds, l1 = h->probe_lds[1] >= 0 ? h->probe_lds[1] : gen_classify_lds_bytes(h->cfg),
                l2 = h->probe_lds[2] >= 0 ? h->probe_lds[2] : h->gen_resolve_lds_bytes;
      if (h->probe_big) {
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenSeedThreads), l0, side, h->probe_us[0], worlds, (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<1>, dim3(wc), dim3(kGenClassifyThreads), l1, side, h->probe_us[1], worlds * gen_classify_parts(h->cfg), (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<1>, dim3(ws), dim3(kGenResolveThreads), l2, side, h->probe_us[2], worlds, (uint32_t*)nullptr);
      } else {
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenSeedThreads), l0, side, h->probe_us[0], worlds, (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(wc), dim3(kGenClassifyThreads), l1, side, h->probe_us[1], worlds * gen_classify_parts(h->cfg), (uint32_t*)nullptr);
        hipLaunchKernelGGL(crafter_gen_occupy_kernel<0>, dim3(ws), dim3(kGenResolveThreads), l2, side, h->probe_us[2], worlds, (uint32_t*)nullptr);
      }
    }
    if (h->plan.gen_geo)
      launch_generation_stamp<1>(h, side, seg, seq);
    else
      launch_generation_stamp<0>(h, side, seg, seq);
  } else
#endif
  if (h->plan.gen_geo)
    launch_generation<1>(h, side, gs, gc, seg, seq, prio);
  else
    launch_generation<0>(h, side, gs, gc, seg, seq, prio);
  e = hipGetLastError();
  if (e != hipSuccess) return pool_fail(h, "generation kernel launch", e);
  // from here on the batch exists: the sequence number is consumed even if a later call fails (its event would then
  // never be trusted, because pool_failed stops the polling)
  h->batches = seq;
  h->steps_since_gen = 0;
  h->gen_parity = (seg + 1) % kGenRing;
  e = hipMemsetAsync(h->st.gen_q + (size_t)seg * gen_q_stride(h->cfg), 0, 16, side);
  if (e != hipSuccess) return pool_fail(h, "hipMemsetAsync(request segment)", e);
  e = hipEventRecord(h->ev_gen[seq % kGenRing], side);
  if (e != hipSuccess) return pool_fail(h, "hipEventRecord(generation stream)", e);
}

// Orders `stream` behind every launched batch (hipStreamWaitEvent: the host does not block) and trusts them all.
static void pool_wait_all(crafter_handle* h, hipStream_t stream, const char* what) {
  for (uint32_t s = h->safe_seq + 1; s <= h->batches && !h->pool_failed; s++) {
    hipError_t ew = hipStreamWaitEvent(stream, h->ev_gen[s % kGenRing], 0);
    if (ew != hipSuccess) pool_fail(h, what, ew);
  }
  if (!h->pool_failed) h->safe_seq = h->batches;
}

// Copies of envs read and write rows of the world pool (crafter_copy_envs: the source's two entries go along; crafter_load_envs:
// the destination's entries are emptied).  Before that every pool row must be at rest, exactly as before crafter_reset: the
// segment collecting requests now is launched as a batch (no request stays queued with PoolHdr.pending set, which would block
// its entry for later requests), the launch stream is ordered behind every launched batch (hipStreamWaitEvent: the host does
// not block) and all of them are trusted.  Batches launched afterwards wait for the copy (ev_main, pool_schedule).
static void pool_quiesce(crafter_handle* h, hipStream_t stream) {
  if (!pool_live(h)) return;
  pool_schedule(h, stream, h->gen_period);
  pool_wait_all(h, stream, "hipStreamWaitEvent(copy)");
}

// A stretch of crafter_step_n / crafter_step_n_envs never crosses a generation batch (requests keep their segment).  Without
// the pool every env that finishes an episode stops in the rollout kernel and runs the REST of the stretch in the regeneration
// kernel, on a small grid, with the generic step instance: stretches stay short there too (one launch over all T
// steps put nearly all the work on that grid once T exceeded an episode).
static int stretch_steps(const crafter_handle* h, int left, bool pooled) {
  int room = pooled ? h->gen_period - h->steps_since_gen : (left < kUnpooledStretch ? left : kUnpooledStretch);
  return left < room ? left : (room > 0 ? room : 1);
}

// A generation batch follows the stretch of T steps: its side stream waits for the stretch's last kernel through that kernel's
// own stop event (pool_schedule main_recorded).
static bool batch_follows(const crafter_handle* h, bool pooled, bool requeue, int T) {
  return pooled && requeue && !h->timing && h->fold_main_event && h->steps_since_gen + T >= h->gen_period;
}
