"""The oracle of authored worlds (tests/worlds_ref.py AuthoredOracle) against the real reference: tests/golden/reference_runs/
authored_world.npz was recorded from the reference with its generate_world replaced at run time by the authored function
(tools/make_worlds_golden.py).  Data only; replayed here on the CPU."""
import numpy as np

from tests import worlds_cases as wc
from tests.parity import GOLDEN, sha8, state_of_snapshot


def test_authored_oracle_replays_the_reference_fixture():
  g = np.load(GOLDEN / 'reference_runs' / 'authored_world.npz')
  k, seed = int(g['case']), int(g['seed'])
  assert np.array_equal(g['actions'], wc.tape(k)), 'the fixture was recorded with another tape'
  run = wc.oracle_run(k, seed)
  fields = ('mat', 'objects', 'inventory', 'achievements', 'misc', 'chunk_order', 'mt_key', 'mt_pos')
  assert np.array_equal(run.frames[0], g['reset_obs'])
  for name, snap in (('reset_', run.snapshots[0]), ('final_', run.snapshots[-1])):
    for f, v in state_of_snapshot(snap).items():
      assert np.array_equal(np.asarray(v), g[name + f]), f'{name}{f}'
  frames = {int(t): fr for t, fr in zip(g['frame_steps'], g['frames'])}
  assert any(t >= 148 for t in frames), 'no night frame in the fixture'
  for t in range(len(g['actions']) + 1):
    s = state_of_snapshot(run.snapshots[t])
    for f in fields:
      assert sha8(s[f]) == g['sha_' + f][t], f'step {t}: {f}'
    assert sha8(run.frames[t]) == g['obs_sha'][t], f'step {t}: frame'
    if t:
      assert run.rewards[t - 1] == g['rewards'][t - 1] and run.dones[t - 1] == bool(g['dones'][t - 1]), f'step {t}: reward / done'
      if t - 1 in frames:
        assert np.array_equal(run.frames[t], frames[t - 1]), f'step {t}: pixels'
