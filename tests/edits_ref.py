"""TEST INFRASTRUCTURE: the reference semantics of an edit between two steps, stated on the oracle.  EditedOracle applies a tape
(crafter_amd.edits.encode's rows, each op valid where it stands: clean_edits' output) with the oracle's own _add / _remove /
_move, `mat[...]`, `inv`, the player's counters and `_step` -- the statements the header names beside each op kind
(include/crafter_hip_edit.h).  The oracle asserts where the reference asserts (World.add / move onto an occupied cell), so a tape
the device would have refused fails here instead of passing quietly.  tests/golden/reference_runs/edits_*.npz ties this to the real reference
(tools/make_edits_golden.py executes the same statements on crafter.Env)."""
import numpy as np

from crafter_amd import abi
from oracle.crafter_oracle import PLAYER, daylight_of
from tests.worlds_ref import AuthoredOracle

WORDS = abi.EDIT_WORDS


def signed_byte(v):
  """health as the object record keeps it."""
  return ((int(v) + 128) & 255) - 128


class EditedOracle(AuthoredOracle):
  """AuthoredOracle (an OracleEnv whose next reset may go into an authored world) with edit(tape)."""

  def edit(self, tape):
    for k, a1, a2, a3, a4, a5, a6, a7 in (tuple(int(v) for v in row) for row in np.asarray(tape).reshape(-1, WORDS)):
      if k == abi.EDIT_NOP:
        continue
      elif k == abi.EDIT_SET_CELL:       # world[x, y] = material  engine.py:82-86
        assert self._inside(a1, a2) and 1 <= a3 <= len(self.t.materials)
        self.mat[a1, a2] = a3
      elif k == abi.EDIT_ADD:            # world.add(cls(world, (x, y)))  engine.py:50-57
        assert abi.T_COW <= a1 <= abi.T_PLANT and self._inside(a2, a3)
        self._add(a1, a2, a3, signed_byte(a4), a5, a6, a7)
      elif k == abi.EDIT_REMOVE:         # world.remove(obj)  engine.py:59-65
        slot = int(self.objmap[a1, a2])
        assert slot > 1
        self._remove(slot)
      elif k == abi.EDIT_MOVE:           # world.move(obj, pos)  engine.py:67-80
        slot = int(self.objmap[a1, a2])
        assert slot >= 1 and self._inside(a3, a4)
        self._move(slot, a3, a4)
      elif k == abi.EDIT_SET_OBJECT:
        slot = int(self.objmap[a1, a2])
        assert slot >= 1 and a3 and not a3 & ~7
        if a3 & abi.EDIT_HEALTH:
          assert self.otype[slot] != PLAYER
          self.ohealth[slot] = signed_byte(a4)
        if a3 & abi.EDIT_FACING:
          assert a5 * a5 + a6 * a6 == 1
          self.ofx[slot], self.ofy[slot] = a5, a6
        if a3 & abi.EDIT_AUX:
          assert self.otype[slot] != PLAYER
          self.oaux[slot] = a7
      elif k == abi.EDIT_SET_ITEM:       # player.inventory[item] = value
        assert 0 <= a2 <= self.t.item_max[a1]
        self.inv[a1] = a2
      elif k == abi.EDIT_SET_PLAYER:     # the counters in half steps, as snapshot() reports them
        name = abi.EDIT_FIELDS[a1]
        lo, hi = abi.EDIT_FIELD_RANGE[name]
        assert lo <= a2 <= hi
        if name == 'sleeping':
          self.sleeping = bool(a2)
        else:
          setattr(self, name[:-1], a2 / 2)
      elif k == abi.EDIT_SET_CLOCK:      # env._step = step; env._update_time()  env.py:135-139
        assert 0 <= a1 and not (self._length and a1 >= self._length)
        self._step = a1
        self.daylight = daylight_of(a1)
      else:
        raise AssertionError(f'no edit op: kind {k}')
