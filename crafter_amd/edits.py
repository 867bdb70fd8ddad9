"""Edits of envs in place: the ops `BatchedEnv.edit(idx, ops)` applies between two steps (include/crafter_hip_edit.h
crafter_edit_envs).  This module is the host side -- building ops, encoding a tape, the Python mirror of the device's refusals --
and needs no device.

An op is what one of the builders returns; a tape is a list of ops, applied in order:

  set_cell(x, y, material)                 world[x, y] = material
  add(cls, x, y, health, facing, aux)      world.add(cls(world, (x, y))), then the fields
  remove(x, y)                             world.remove(world[x, y][1])
  move(x, y, x2, y2)                       world.move(world[x, y][1], (x2, y2))          (the player too: a teleport)
  set_object(x, y, health, facing, aux)    obj.health / obj.facing / obj.cooldown | reload | grown = ...
  set_item(item, value)                    player.inventory[item] = value
  set_player(sleeping=, hunger2=, ...)     player.sleeping, _hunger, _thirst, _fatigue, _recover (snapshot()'s units)
  set_clock(step)                          env._step = step; env._update_time()

Materials, classes and items are names or ids, as crafter_amd.WorldBank takes them."""
import numpy as np

from . import abi
from .worlds import CLASS_HEALTH, CLASS_IDS, CLASS_NAMES, _geometry

WORDS = abi.EDIT_WORDS
NOP = (abi.EDIT_NOP,)


class Ops(list):
  """Several ops that stand where one does in a tape (set_player's return)."""


def set_cell(x, y, material):
  return (abi.EDIT_SET_CELL, x, y, material)


def add(cls, x, y, health=None, facing=(0, 1), aux=0):
  """health None: what a fresh object of the class has (objects.py:266, 285, 318, 391).  Only an arrow keeps its facing."""
  return (abi.EDIT_ADD, cls, x, y, health, facing, aux)


def remove(x, y):
  return (abi.EDIT_REMOVE, x, y)


def move(x, y, x2, y2):
  return (abi.EDIT_MOVE, x, y, x2, y2)


def set_object(x, y, health=None, facing=None, aux=None):
  """Assigns the fields that are not None.  aux is the zombie's cooldown, the skeleton's reload, the plant's `grown`."""
  return (abi.EDIT_SET_OBJECT, x, y, health, facing, aux)


def set_item(item, value):
  return (abi.EDIT_SET_ITEM, item, value)


def set_player(**fields):
  """One op per field, in the order given: sleeping, hunger2, thirst2, fatigue2, recover2."""
  return Ops((abi.EDIT_SET_PLAYER, name, value) for name, value in fields.items())


def set_clock(step):
  return (abi.EDIT_SET_CLOCK, step)


def _limits(batch_or_geometry):
  """-> (W, H, rules, n_daylight or None, length or None) of a batch, or of dict(area=, rules=, n_daylight=, length=)."""
  W, H, rules = _geometry(batch_or_geometry)
  g = batch_or_geometry
  if isinstance(g, dict):
    return W, H, rules, g.get('n_daylight'), g.get('length')
  return W, H, rules, int(g.cfg.n_daylight), int(g.cfg.length) or None


def _flat(ops):
  """A tape with set_player's lists spliced in."""
  out = []
  for op in ops:
    if isinstance(op, Ops):
      out.extend(op)
    else:
      out.append(op)
  return out


def _id(value, names, what, first=0):
  """A name of `names` or an integer id -> the id (first: the id of names[0])."""
  if isinstance(value, str):
    if value not in names:
      raise ValueError(f'unknown {what} {value!r}')
    return first + list(names).index(value)
  if not isinstance(value, (int, np.integer)):
    raise ValueError(f'a {what} is a name or an integer id, got {value!r}')
  return int(value)


def _int(v, op, what):
  """An integer value of an op (bools count: sleeping=True) -> int; anything else, a float in range included, is no value."""
  if not isinstance(v, (int, np.integer)):
    raise ValueError(f'{op!r}: {what} must be an integer, got {v!r}')
  return int(v)


def _row(op, W, H, rules, n_daylight, length, validate):
  """One op -> its eight words.  validate: everything the device would flag that can be seen without the state raises ValueError."""
  op = tuple(op)
  if not op or not isinstance(op[0], (int, np.integer)) or not 0 <= op[0] < abi.EDIT_KINDS:
    raise ValueError(f'no edit op: {op!r} (use the builders of crafter_amd.edits)')
  kind, words = int(op[0]), [0] * (WORDS - 1)
  materials, items = list(rules['materials']), list(rules['items'])

  def cell(x, y):
    x, y = _int(x, op, 'a cell coordinate'), _int(y, op, 'a cell coordinate')
    if validate and not (0 <= x < W and 0 <= y < H):
      raise ValueError(f'{op!r}: cell ({x}, {y}) lies outside the {W} x {H} world')
    return x, y

  def facing_of(f, needs_axis):
    fx, fy = (_int(v, op, 'a facing component') for v in f)
    if validate and needs_axis and fx * fx + fy * fy != 1:
      raise ValueError(f'{op!r}: facing ({fx}, {fy}) is no unit axis vector')
    return fx, fy

  want = {abi.EDIT_NOP: 1, abi.EDIT_SET_CELL: 4, abi.EDIT_ADD: 7, abi.EDIT_REMOVE: 3, abi.EDIT_MOVE: 5, abi.EDIT_SET_OBJECT: 6,
          abi.EDIT_SET_ITEM: 3, abi.EDIT_SET_PLAYER: 3, abi.EDIT_SET_CLOCK: 2}[kind]
  if len(op) != want:
    raise ValueError(f'no edit op: {op!r} (use the builders of crafter_amd.edits)')
  if kind == abi.EDIT_SET_CELL:
    m = _id(op[3], materials, 'material', 1)
    if validate and not 1 <= m <= len(materials):
      raise ValueError(f'{op!r}: material ids lie in 1 .. {len(materials)}')
    words[:3] = [*cell(op[1], op[2]), m]
  elif kind == abi.EDIT_ADD:
    cls = op[1]
    typ = CLASS_IDS.get(cls.lower(), None) if isinstance(cls, str) else _id(cls, (), 'object class')
    if typ is None:
      raise ValueError(f'unknown object class {cls!r} (one of {CLASS_NAMES})')
    if validate and not abi.T_COW <= typ <= abi.T_PLANT:
      raise ValueError(f'{op!r}: only cow, zombie, skeleton, arrow and plant can be added')
    health = CLASS_HEALTH.get(typ, 0) if op[4] is None else _int(op[4], op, 'health')
    if validate and not -128 <= health <= 127:
      raise ValueError(f'{op!r}: health does not fit the record\'s signed byte')
    fx, fy = facing_of(op[5], typ == abi.T_ARROW) if typ == abi.T_ARROW else (0, 0)   # (the other classes keep none)
    words[:7] = [typ, *cell(op[2], op[3]), health, fx, fy, _int(op[6], op, 'aux')]
  elif kind == abi.EDIT_REMOVE:
    words[:2] = cell(op[1], op[2])
  elif kind == abi.EDIT_MOVE:
    words[:4] = [*cell(op[1], op[2]), *cell(op[3], op[4])]
  elif kind == abi.EDIT_SET_OBJECT:
    health, facing, aux = op[3:6]
    health, aux = (None if v is None else _int(v, op, what) for v, what in ((health, 'health'), (aux, 'aux')))
    which = (abi.EDIT_HEALTH if health is not None else 0) | (abi.EDIT_FACING if facing is not None else 0) | (
        abi.EDIT_AUX if aux is not None else 0)
    if validate and health is not None and not -128 <= health <= 127:
      raise ValueError(f'{op!r}: health does not fit the record\'s signed byte')
    fx, fy = facing_of(facing, True) if facing is not None else (0, 0)
    words[:7] = [*cell(op[1], op[2]), which, health or 0, fx, fy, aux or 0]
  elif kind == abi.EDIT_SET_ITEM:
    item = _id(op[1], items, 'item')
    if validate and not 0 <= item < len(items):
      raise ValueError(f'{op!r}: item ids lie in 0 .. {len(items) - 1}')
    most = int(rules['items'][items[item]]['max']) if 0 <= item < len(items) else 0
    value = _int(op[2], op, 'an item count')
    if validate and not 0 <= value <= most:
      raise ValueError(f'{op!r}: {items[item]} lies in 0 .. {most}')
    words[:2] = [item, value]
  elif kind == abi.EDIT_SET_PLAYER:
    field = _id(op[1], abi.EDIT_FIELDS, 'player field')
    if validate and not 0 <= field < len(abi.EDIT_FIELDS):
      raise ValueError(f'{op!r}: player fields are {abi.EDIT_FIELDS}')
    value = _int(op[2], op, 'a field value')
    if validate:
      lo, hi = abi.EDIT_FIELD_RANGE[abi.EDIT_FIELDS[field]]
      if not lo <= value <= hi:
        raise ValueError(f'{op!r}: {abi.EDIT_FIELDS[field]} lies in {lo} .. {hi}')
    words[:2] = [field, value]
  elif kind == abi.EDIT_SET_CLOCK:
    step = _int(op[1], op, 'the step')
    if validate and (step < 0 or (n_daylight is not None and step >= n_daylight) or (length and step >= length)):
      raise ValueError(f'{op!r}: the step lies in 0 .. min(daylight table, length) - 1')
    words[0] = step
  for v in words:
    if not -2 ** 31 <= v < 2 ** 31:
      raise ValueError(f'{op!r}: a value does not fit an int32 word')
  return [kind] + words


def encode(batch_or_rules, ops, n, validate=True):
  """ops: a list of n tapes (one per named env), or ONE tape applied to every named env -> the device's form, np.int32
  [n, L, 8] padded with NOP (L >= 1).  Callable without a device: batch_or_rules is a BatchedEnv (or anything with .cfg and
  .rules) or dict(area=(W, H), rules=None, n_daylight=None, length=None).  Everything the device would flag (ST_BAD_EDIT) that
  can be seen without the state raises ValueError here; validate=False skips those checks and leaves them to the device."""
  W, H, rules, n_daylight, length = _limits(batch_or_rules)
  ops = list(ops)
  one = all(isinstance(o, (tuple, Ops)) for o in ops)   # (a tape is a plain list)
  tapes = [ops] * n if one else ops
  if len(tapes) != n:
    raise ValueError(f'{len(tapes)} tapes for {n} envs')
  rows = [[_row(op, W, H, rules, n_daylight, length, validate) for op in _flat(t)] for t in tapes]
  L = max([len(r) for r in rows] + [1])
  out = np.zeros((n, L, WORDS), np.int32)
  for i, r in enumerate(rows):
    if r:
      out[i, :len(r)] = np.array(r, np.int64).astype(np.int32)
  return out


def clean_edits(batch_or_rules, snapshot, tape):
  """The Python mirror of the device's refusals (include/crafter_hip_edit.h): what crafter_edit_envs makes of `tape` -- np.int32
  [L, 8], one env's row of encode() -- on an env whose state is `snapshot` (a snapshot() dict: 'objects' decides which cells are
  occupied) -> (tape, flagged): the ops that are applied, each one valid where it stands, repaired where the device repairs, and
  whether ST_BAD_EDIT is set.  A full slot table (ST_OBJ_OVERFLOW) is not modelled."""
  W, H, rules, n_daylight, length = _limits(batch_or_rules)
  n_materials, items = len(rules['materials']), list(rules['items'])
  item_max = [int(rules['items'][k]['max']) for k in items]
  inside = lambda x, y: 0 <= x < W and 0 <= y < H
  axis = lambda fx, fy: fx * fx + fy * fy == 1
  byte = lambda v: ((int(v) + 128) & 255) - 128
  at = {(o[1], o[2]): o[0] for o in snapshot['objects']}   # cell -> class
  out, flagged = [], False
  for k, a1, a2, a3, a4, a5, a6, a7 in (tuple(int(v) for v in row) for row in np.asarray(tape).reshape(-1, WORDS)):
    bad = False
    if k == abi.EDIT_NOP:
      continue
    elif k == abi.EDIT_SET_CELL:
      if inside(a1, a2) and 1 <= a3 <= n_materials:
        out.append([k, a1, a2, a3, 0, 0, 0, 0])
      else:
        bad = True
    elif k == abi.EDIT_ADD:
      if abi.T_COW <= a1 <= abi.T_PLANT and inside(a2, a3) and (a2, a3) not in at:
        fx, fy = (a5, a6) if a1 == abi.T_ARROW else (0, 0)
        if a1 == abi.T_ARROW and not axis(fx, fy):
          bad, fx, fy = True, 0, 1
        at[(a2, a3)] = a1
        out.append([k, a1, a2, a3, byte(a4), fx, fy, a7])
      else:
        bad = True
    elif k == abi.EDIT_REMOVE:
      if inside(a1, a2) and at.get((a1, a2), abi.T_PLAYER) != abi.T_PLAYER:
        del at[(a1, a2)]
        out.append([k, a1, a2, 0, 0, 0, 0, 0])
      else:
        bad = True
    elif k == abi.EDIT_MOVE:
      if not (inside(a1, a2) and (a1, a2) in at and inside(a3, a4)):
        bad = True
      elif (a3, a4) != (a1, a2):
        if (a3, a4) in at:
          bad = True
        else:
          at[(a3, a4)] = at.pop((a1, a2))
          out.append([k, a1, a2, a3, a4, 0, 0, 0])
    elif k == abi.EDIT_SET_OBJECT:
      if inside(a1, a2) and (a1, a2) in at:
        typ, which = at[(a1, a2)], a3
        known = abi.EDIT_HEALTH | abi.EDIT_FACING | abi.EDIT_AUX
        if which & ~known:
          bad, which = True, which & known
        if typ == abi.T_PLAYER and which & (abi.EDIT_HEALTH | abi.EDIT_AUX):
          bad, which = True, which & abi.EDIT_FACING
        if which & abi.EDIT_FACING:
          if typ not in (abi.T_PLAYER, abi.T_ARROW):
            which &= ~abi.EDIT_FACING
          elif not axis(a5, a6):
            bad, which = True, which & ~abi.EDIT_FACING
        if which:
          out.append([k, a1, a2, which, byte(a4) if which & abi.EDIT_HEALTH else 0, a5 if which & abi.EDIT_FACING else 0,
                      a6 if which & abi.EDIT_FACING else 0, a7 if which & abi.EDIT_AUX else 0])
      else:
        bad = True
    elif k == abi.EDIT_SET_ITEM:
      if 0 <= a1 < len(items):
        v = min(max(a2, 0), item_max[a1])
        bad = v != a2
        out.append([k, a1, v, 0, 0, 0, 0, 0])
      else:
        bad = True
    elif k == abi.EDIT_SET_PLAYER:
      if 0 <= a1 < len(abi.EDIT_FIELDS) and abi.EDIT_FIELD_RANGE[abi.EDIT_FIELDS[a1]][0] <= a2 <= abi.EDIT_FIELD_RANGE[abi.EDIT_FIELDS[a1]][1]:
        out.append([k, a1, a2, 0, 0, 0, 0, 0])
      else:
        bad = True
    elif k == abi.EDIT_SET_CLOCK:
      if a1 >= 0 and (n_daylight is None or a1 < n_daylight) and not (length and a1 >= length):
        out.append([k, a1, 0, 0, 0, 0, 0, 0])
      else:
        bad = True
    else:
      bad = True
    flagged |= bad
  return np.array(out, np.int32).reshape(-1, WORDS), flagged
