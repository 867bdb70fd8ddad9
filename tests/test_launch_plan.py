"""CPU tests of the launch rule (csrc/launch_plan.hpp): which step / rollout instance a handle runs, in how much LDS, and
which kernel one crafter_step call launches.  The CPU harness exports the header's functions as they are
(hostsim_launch_plan); the library and the harness's own stepping go through the same ones."""
import copy
import ctypes as C
import itertools
import types

import pytest

from crafter_amd import tables
from tests.hostsim import driver

RULES = tables.load_rules()
OTHER_RULES = copy.deepcopy(RULES)
OTHER_RULES['items']['health'] = {'max': 5, 'initial': 5}   # (run_random.py:21-22)
OTHER_VIEW = dict(view=(7, 9), size=(84, 72))

# name: (rules, make_config arguments, instance, instance before the tables are uploaded,
#        (step, rollout, reset, render) LDS bytes of the launches -- printed from the layout functions of env_kernels.hpp
#        before the plan existed: lds_layout(c, 1, false, false) / lds_layout(c, 1) / lds_layout(c) / big_layout(c) totals,
#        big_reset_layout(c).total, lds_layout(c).total)
CASES = {
    'default': (RULES, {}, 7, 6, (24848, 24848, 33664, 33664)),
    'other-rules': (OTHER_RULES, {}, 6, 6, (25168, 25168, 33664, 33664)),
    'area32': (RULES, dict(area=(32, 32)), 4, 4, (23840, 23840, 23840, 23840)),
    'size100x72': (RULES, dict(size=(100, 72)), 4, 4, (37184, 37184, 37184, 37184)),
    'objects512': (RULES, dict(max_objects=512), 4, 4, (37760, 37760, 37760, 37760)),
    'area256': (RULES, dict(area=(256, 256)), 9, 0, (15504, 15504, 27584, 72704)),
    'area256-other-view': (RULES, dict(area=(256, 256), **OTHER_VIEW), 0, 0, (11040, 11040, 23120, 72016)),
    'area256-other-rules': (OTHER_RULES, dict(area=(256, 256)), 0, 0, (15504, 15504, 27584, 72704)),
}
FIELDS = ('instance', 'maps_in_lds', 'gen_geo', 'step_lds', 'rollout_lds', 'render_lds', 'reset_lds', 'night_px', 'opt_in_lds',
          'kernel', 'ordered', 'early_frame')
KERNELS = ('crafter_step_kernel', 'crafter_step_early_kernel', 'crafter_step_wide_kernel', 'crafter_rules_kernel',
           'crafter_rules_kernel + crafter_frame_kernel')   # launch_plan.hpp StepKernel
NUM_ENVS = (1, 512, 513, 1280, 1281, 2047, 2048, 4096, 16384, 16385)


def plan(name, have_tables=True, num_envs=8, frames=True, order=-1, split=-1, wide=-1, early=-1, lds_pad=0, rollout_lds_pad=0):
  rules, kw = CASES[name][:2]
  lib = driver.lib()
  cfg, _ = tables.make_config(num_envs, rules, **kw)
  default_rules = lib.hostsim_is_default_rules(C.byref(tables.build_rules(rules)))
  out = (C.c_int32 * len(FIELDS))()
  lib.hostsim_launch_plan(C.byref(cfg), int(have_tables), default_rules, num_envs, int(frames), order, split, wide, early, lds_pad,
                          rollout_lds_pad, out)
  return types.SimpleNamespace(**dict(zip(FIELDS, out)))


def instance_name(k):
  """BatchedEnv.step_instance of a handle whose crafter_step_instance() is k"""
  from crafter_amd.batched import BatchedEnv
  fake = types.SimpleNamespace(_lib=types.SimpleNamespace(crafter_step_instance=lambda h: k), _handle=None)
  return BatchedEnv.step_instance.fget(fake)


@pytest.mark.parametrize('name', list(CASES))
def test_instances_and_lds_bytes(name):
  _, _, instance, before, (step, rollout, reset, render) = CASES[name]
  p = plan(name)
  assert p.instance == instance and plan(name, have_tables=False).instance == before
  assert instance_name(p.instance) == {7: 'crafter_step_kernel<1, 1, 1>', 6: 'crafter_step_kernel<1, 1, 0>', 4: 'crafter_step_kernel<1, 0, 0>',
                                       9: 'crafter_step_kernel<0, 2, 1>', 0: 'crafter_step_kernel<0, 0, 0>'}[instance]
  assert (p.step_lds, p.rollout_lds, p.reset_lds, p.render_lds) == (step, rollout, reset, render)
  big = instance in (0, 9)
  assert p.maps_in_lds == (not big) and p.night_px == big and p.gen_geo == (instance in (6, 7))
  assert p.opt_in_lds == (render > 64 * 1024)
  # the pads of probe builds: CRAFTER_LDS_PAD on every step launch and on the rollouts that launch in the step's bytes,
  # CRAFTER_ROLLOUT_LDS_PAD on the resident rollout of the default instance alone, neither on the generic LDS-resident rollout
  q = plan(name, lds_pad=8, rollout_lds_pad=24)
  assert q.step_lds == step + 8
  assert q.rollout_lds == rollout + {7: 24, 6: 8, 0: 8, 9: 8, 4: 0}[instance]
  assert (q.reset_lds, q.render_lds, q.instance) == (reset, render, instance)


@pytest.mark.parametrize('name', ['default', 'area32', 'area256'])
def test_kernel_choice_is_what_bench_states(name, monkeypatch):
  """bench.step_kernel_name states the rule independently (it does not model the dispatch order: a forced wide kernel is
  compared where no order is kept)."""
  import bench
  inst = instance_name(plan(name).instance)
  knobs = ('CRAFTER_SPLIT', 'CRAFTER_STEP_WIDE', 'CRAFTER_STEP_EARLY')
  monkeypatch.delenv('CRAFTER_ORDER', raising=False)
  for values in itertools.product((None, 0, 1), repeat=3):
    for k, v in zip(knobs, values):
      monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, str(v))
    split, wide, early = (-1 if v is None else v for v in values)
    for n, render in itertools.product(NUM_ENVS, (False, True)):
      if wide == 1 and n > 1280:
        continue
      p = plan(name, num_envs=n, frames=render, split=split, wide=wide, early=early)
      want = bench.step_kernel_name(types.SimpleNamespace(step_instance=inst, num_envs=n), render)
      assert KERNELS[p.kernel] == want, (values, n, render)
      assert p.early_frame == (early if early >= 0 else int(n >= 2048))   # StepCtl::early_frame, whichever kernel runs


def test_an_ordered_launch_is_never_the_wide_kernel():
  for n in NUM_ENVS:   # the order is kept from 1281 to 16384 envs ...
    assert plan('default', num_envs=n).ordered == (1280 < n <= 16384)
    assert plan('default', num_envs=n, order=1).ordered == (n <= 16384)   # ... with CRAFTER_ORDER=1 from one env on
    assert not plan('default', num_envs=n, order=0).ordered
    forced = plan('default', num_envs=n, wide=1)
    if forced.ordered:   # CRAFTER_STEP_WIDE=1 does not reach an ordered launch
      assert KERNELS[forced.kernel] == ('crafter_step_early_kernel' if n >= 2048 else 'crafter_step_kernel')
    else:
      assert KERNELS[forced.kernel] == 'crafter_step_wide_kernel'
    assert KERNELS[plan('default', num_envs=n, wide=1, order=1).kernel] == (
        'crafter_step_wide_kernel' if n > 16384 else 'crafter_step_early_kernel' if n >= 2048 else 'crafter_step_kernel')
  assert KERNELS[plan('default', num_envs=8).kernel] == 'crafter_step_wide_kernel'
  assert KERNELS[plan('default', num_envs=8, order=1).kernel] == 'crafter_step_kernel'
  # the split pair follows no order; every other instance runs its fused kernel, ordered or not
  assert not plan('default', num_envs=4096, frames=False).ordered and not plan('default', num_envs=4096, split=1).ordered
  assert plan('area32', num_envs=4096, frames=False).ordered and KERNELS[plan('area32', num_envs=4096, frames=False).kernel] == 'crafter_step_kernel'
