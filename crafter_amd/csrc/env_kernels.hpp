// Bodies of the two per-environment kernels (one workgroup = one environment):
//   step_body  : Env.step  (env.py:83-118)  -> dynamics, balance, reward/done, obs render
//   reset_body : Env.reset (env.py:70-81)   -> reseed, worldgen, first obs
// plus the LDS carve-up and the HBM <-> LDS staging they share.
//
// HBM layout is struct-of-arrays over envs (types.hpp StatePtrs).  A kernel stages one env's
// working set into LDS, runs the rules there, writes map changes through to HBM as they happen
// and stores the compact tables (slot table, MT key, scalar record, chunk order) on exit.
// The text lives in one header per concern; this one includes them all:
//   lds_layout.hpp    geometry predicates, every LDS layout (sizes and offsets, shared with the host)
//   env_stage.hpp     bind_lds, load_env / store_env, the material window, share_registers, noise_chain, obs_target, write_semantic
//   pool_entry.hpp    the world-pool protocol on the device: gen_wanted ... adopt_world
//   step_body.hpp     StepCtl, the frame record, frame_body, step_body, rollout_body
//   reset_bodies.hpp  the reset skeleton and its callers, requeue_rollout_body, render_body, final_reset_body
//   gen_bodies.hpp    gen_body, gen_seed_body, gen_classify_body, gen_resolve_body
#pragma once
#include "lds_layout.hpp"
#include "env_stage.hpp"
#include "pool_entry.hpp"
#include "step_body.hpp"
#include "reset_bodies.hpp"
#include "gen_bodies.hpp"
