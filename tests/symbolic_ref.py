"""The symbolic observation (BatchedEnv.symbolic, include/crafter_hip.h crafter_symbolic) restated in plain Python from an
OracleEnv -- semantic(), objects(), inv, sleeping, daylight -- and the tapes the symbolic tests share.

local uint8 [2, gw, gh]: cell (x, y) is world cell player.pos + (x, y) - (gw // 2, gh // 2) (engine.py:155-187); plane 0 the
semantic id there (engine.py:251-264), 0 outside the world; plane 1 the sprite variant of the object on it
(objects.py:85-93, 361-367, 395-403).  stats float32 [n_items + 4]: inventory, facing x, facing y, sleeping, daylight."""
import numpy as np

from tests import scenarios

PLAYER, COW, ZOMBIE, SKELETON, ARROW, PLANT = 1, 2, 3, 4, 5, 6
FACING = {(-1, 0): 1, (1, 0): 2, (0, -1): 3, (0, 1): 4}

# (kind, seed, steps, area, steps before which every live plant's `grown` is set to 301).  planter: at step 200 this tape has
# no plant alive (the player has eaten them all), so the poke is applied at step 100 as well, where five stand.
CASES = {
    'sleeper': ('sleeper', 7, 300, (64, 64), ()),
    'fighter': ('fighter', 5, 200, (16, 16), ()),
    'planter': ('planter', 5, 400, (64, 64), (100, 200)),
}
RIPE = 301


def variant(typ, fx, fy, aux, sleeping):
  if typ == PLAYER:
    return 5 if sleeping else FACING[(fx, fy)]
  if typ == ARROW:
    return FACING[(fx, fy)]
  if typ == PLANT:
    return 1 if aux > 300 else 0
  return 0


def symbolic_of(orc):
  """-> (local u8 [2, gw, gh], stats f32 [n_items + 4]) of the oracle's current state."""
  gw, gh = (int(v) for v in orc._local_grid)
  W, H = orc._area
  sem = orc.semantic()
  objs = orc.objects()
  assert objs[0][0] == PLAYER
  px, py = objs[0][1], objs[0][2]
  local = np.zeros((2, gw, gh), np.uint8)
  for x in range(gw):
    for y in range(gh):
      wx, wy = px + x - gw // 2, py + y - gh // 2
      if 0 <= wx < W and 0 <= wy < H:
        local[0, x, y] = sem[wx, wy]
  for typ, ox, oy, _, fx, fy, aux in objs:
    x, y = ox - px + gw // 2, oy - py + gh // 2
    if 0 <= x < gw and 0 <= y < gh:
      local[1, x, y] = variant(typ, fx, fy, aux, orc.sleeping)
  stats = np.array(list(orc.inv) + [objs[0][4], objs[0][5], int(bool(orc.sleeping))], np.float32)
  return local, np.concatenate([stats, np.array([orc.daylight], np.float64).astype(np.float32)])


def names(rules):
  """(class names indexed by the plane-0 id, column names of stats)."""
  classes = ['none'] + list(rules['materials']) + ['player', 'cow', 'zombie', 'skeleton', 'arrow', 'plant']
  return classes, list(rules['items']) + ['facing_x', 'facing_y', 'sleeping', 'daylight']


def tape(case):
  kind, seed, steps, area, poke = CASES[case]
  acts, gifts = scenarios.SCENARIOS[kind](steps, seed)
  return acts, gifts, seed, area, poke


def gift_oracle(orc, gift):
  items = list(orc.t.items)
  for item, amount in gift.items():
    orc.inv[items.index(item)] = amount


def poke_oracle(orc):
  for s in range(1, len(orc.otype)):
    if orc.otype[s] == PLANT:
      orc.oaux[s] = RIPE


def poke_objs(objs_view, nobj):
  """Sets `aux` (grown) of every live plant in one env's slot table (crafter_amd.state.objs_view record array) to RIPE."""
  for s in range(1, int(nobj)):
    if objs_view['type'][s] == PLANT:
      objs_view['aux'][s] = RIPE


def oracle_run(case, area=None, view=(9, 9), size=(64, 64), steps=None):
  """-> (a reset OracleEnv for the case, its actions, its gifts {step: {item: amount}}, its poke steps): the caller
  applies gifts[t] and the poke to both sides before step t (gift_oracle / poke_oracle on this one)."""
  from oracle.crafter_oracle import OracleEnv
  acts, gifts, seed, case_area, poke = tape(case)
  orc = OracleEnv(area=area or case_area, view=view, size=size, seed=seed)
  orc.reset()
  return orc, acts[:steps], gifts, poke


def oracle_trace(case, **kw):
  """-> (locals u8 [T + 1, 2, gw, gh], stats f32 [T + 1, n + 4]) of the case on the oracle: after reset, then after every step."""
  orc, acts, gifts, poke = oracle_run(case, **kw)
  out = [symbolic_of(orc)]
  for t, a in enumerate(acts):
    if t in gifts:
      gift_oracle(orc, gifts[t])
    if t in poke:
      poke_oracle(orc)
    orc.step(int(a))
    out.append(symbolic_of(orc))
  return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
