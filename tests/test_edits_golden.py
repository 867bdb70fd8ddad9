"""The oracle of edits in place (tests/edits_ref.py EditedOracle) against the real reference: tests/golden/reference_runs/
edits_<case>.npz were recorded from the reference with the statements of include/crafter_hip_edit.h executed on crafter.Env
between the steps the cases' schedules name (tools/make_edits_golden.py).  Data only; replayed here on the CPU."""
import numpy as np
import pytest

from tests import edits_cases as ec
from tests.parity import GOLDEN, sha8, state_of_snapshot

FIELDS = ('mat', 'objects', 'inventory', 'achievements', 'misc', 'chunk_order', 'mt_key', 'mt_pos')


@pytest.mark.parametrize('k', range(3))
def test_edited_oracle_replays_the_reference_fixture(k):
  g = np.load(GOLDEN / 'reference_runs' / f'edits_{k}.npz')
  assert int(g['case']) == k and int(g['seed']) == ec.SEEDS[k]
  assert np.array_equal(g['actions'], ec.tape(k)), 'the fixture was recorded with another tape'
  assert list(g['edit_steps']) == sorted(ec.SCHEDULES[k]), 'the fixture was recorded with another schedule'
  run = ec.oracle_run(k, ec.SEEDS[k])
  for name, snap in (('reset_', run.snapshots[0]), ('final_', run.snapshots[-1])):
    for f, v in state_of_snapshot(snap).items():
      assert np.array_equal(np.asarray(v), g[name + f]), f'{name}{f}'
  for j, t in enumerate(g['edit_steps']):
    s = state_of_snapshot(run.edited[int(t)])
    for f in FIELDS:
      assert sha8(s[f]) == g['edited_sha_' + f][j], f'behind the edit before step {t + 1}: {f}'
  for t in range(len(g['actions']) + 1):
    s = state_of_snapshot(run.snapshots[t])
    for f in FIELDS:
      assert sha8(s[f]) == g['sha_' + f][t], f'step {t}: {f}'
    assert run.snapshots[t]['step'] == g['steps'][t], f'step {t}: the clock'
    assert sha8(run.frames[t]) == g['obs_sha'][t], f'step {t}: frame'
    if t:
      assert run.rewards[t - 1] == g['rewards'][t - 1] and run.dones[t - 1] == bool(g['dones'][t - 1]), f'step {t}: reward / done'
