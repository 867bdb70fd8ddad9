"""BatchedEnv: N Crafter environments resident on one MI355X, stepped by libcrafter_hip.so.

This is the batched form of the reference's ``crafter.Env`` (env.py:25-133): same constructor
arguments per environment, ``reset()`` / ``step(actions)`` / ``render()`` over tensors.  All world
state lives in caller-owned torch tensors on the GPU (struct-of-arrays, crafter_hip_types.h crafter_state_ptrs); this
class only allocates them, uploads the host-evaluated tables and enqueues kernels on the current
torch stream.  There is no CPU implementation behind it.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

from . import abi, lib as _libmod, state, tables, worlds as _worlds

_TORCH_DTYPE = {np.uint8: torch.uint8, np.uint16: torch.int16, np.uint32: torch.int32, np.int32: torch.int32, np.float32: torch.float32}


class CrafterDeviceError(RuntimeError):
  pass


def _ptr(t):
  """A tensor's address as the void* the C ABI takes; None (an argument left out) stays None."""
  return None if t is None else C.c_void_p(t.data_ptr())


def _on_device(t):
  return torch.is_tensor(t) and t.is_cuda


class EnvStore:
  """Copies of env rows taken by BatchedEnv.save_state: each env's state (no world-pool buffers, no queues) and its last obs /
  reward / done, in device tensors (or host tensors after .cpu(), e.g. for pickling), with the geometry they were taken with.
  BatchedEnv.load_state writes them into rows of any batch of the same geometry."""

  def __init__(self, tensors, geometry, idx):
    self.tensors = tensors
    self.geometry = dict(geometry)
    self.idx = idx   # the rows the store was taken from (load_state's default destination)

  def __len__(self):
    return int(self.tensors['rec'].shape[0])

  @property
  def device(self):
    return self.tensors['rec'].device

  @property
  def max_objects(self):
    return int(self.tensors['objs'].shape[1])

  def to(self, device):
    return EnvStore({k: v.to(device) for k, v in self.tensors.items()}, self.geometry, self.idx)

  def cpu(self):
    return self.to('cpu')

  def _ptrs(self):
    ptrs = {name: None for name, _ in abi.StatePtrs._fields_}
    ptrs.update({k: v.data_ptr() for k, v in self.tensors.items() if k in ptrs})
    return abi.StatePtrs(**ptrs)


class _Handle:
  """One crafter_handle: config + uploaded tables (+ the state buffers bound to it)."""

  def __init__(self, lib, cfg, host_tables, device):
    self.lib, self.cfg, self.tables, self.device = lib, cfg, host_tables, device
    self._pid = os.getpid()   # the handle belongs to this process: a forked child must never call into HIP with it
    self.ptr = C.c_void_p()
    with torch.cuda.device(device):
      if lib.crafter_create(C.byref(cfg), C.byref(self.ptr)):
        raise CrafterDeviceError(_libmod.last_error(lib, None))
      self._rules_buf = host_tables.rules_bytes()
      ht = _libmod.HostTablesC()
      for name, ctype in ht._fields_:
        if name == 'rules':
          ht.rules = self._rules_buf.ctypes.data
        elif name == 'atlas_bytes':
          ht.atlas_bytes = host_tables.atlas.nbytes
        elif ctype is C.c_void_p:   # table x of the host tables, followed by its length n_x
          setattr(ht, name, getattr(host_tables, name).ctypes.data)
        else:
          setattr(ht, name, getattr(host_tables, name[2:]).size)
      self.check(lib.crafter_upload_tables(self.ptr, C.byref(ht)))

  def check(self, rc):
    if rc:
      raise CrafterDeviceError(_libmod.last_error(self.lib, self.ptr))

  def bind(self, state_ptrs):
    self.check(self.lib.crafter_bind_state(self.ptr, C.byref(state_ptrs)))

  def close(self):
    if self.ptr and self.ptr.value and os.getpid() == self._pid:
      self.lib.crafter_destroy(self.ptr)
    self.ptr = C.c_void_p()


class BatchedEnv:

  def __init__(self, num_envs, area=(64, 64), view=(9, 9), size=(64, 64), reward=True, length=10000,
               seed=None, seeds=None, device='cuda', auto_reset=True, semantic=False, render=True,
               max_objects=None, rules=None, textures=None, gen_period=0, grow_objects=True):
    if not torch.cuda.is_available():
      raise CrafterDeviceError('BatchedEnv needs a HIP device (torch.cuda.is_available() is False); '
                               'there is no CPU path')
    self._lib = _libmod.load()
    self.device = torch.device(device)
    if self.device.type != 'cuda':
      raise CrafterDeviceError(f'device must be a GPU, got {device!r}')
    if self.device.index is None:
      self.device = torch.device('cuda', torch.cuda.current_device())
    self.num_envs = int(num_envs)
    if seeds is None:
      if seed is None:
        seeds = [int(np.random.randint(0, 2 ** 31 - 1)) for _ in range(self.num_envs)]  # env.py:32
      else:
        seeds = [seed + i for i in range(self.num_envs)]
    self.seeds = list(seeds)
    if len(self.seeds) != self.num_envs:
      raise ValueError('len(seeds) != num_envs')
    self.rules = rules or tables.load_rules()
    self.cfg, self.geo = tables.make_config(
        self.num_envs, self.rules, area, view, size, reward, length, max_objects=max_objects,
        auto_reset=auto_reset, want_semantic=semantic, render_obs=render)
    self.cfg.step_threads = 0    # workgroup sizes are compile-time constants of the library
    self.cfg.reset_threads = 0
    self.cfg.gen_period = int(gen_period)   # world pool: 0 = default, < 0 = off (auto-reset always regenerates inline)
    self.tables = tables.HostTables(self.rules, textures or tables.load_textures(), self.cfg, self.geo)
    self._ctor = dict(area=area, view=view, reward=reward, length=length, max_objects=self.cfg.max_objects)
    self.action_names = list(self.rules['actions'])
    self.item_names = list(self.rules['items'])
    self.achievement_names = list(self.rules['achievements'])
    self._textures = textures or tables.load_textures()
    self._native = _Handle(self._lib, self.cfg, self.tables, self.device)
    self._handle = self._native.ptr
    self._aux = {}   # render(size) handles for other frame sizes, bound to the same state
    self._levels = None   # set_levels: the level table's device tensors
    self._final = None   # final_buffers: what step(final=True) writes
    self._prof = None   # enable_phase_stamps: the stamp buffer
    self._timing_on = False
    self.objects_grown = 0   # times _grow_objects doubled the slot table
    self._keep = None   # the tensors of the last call enqueued: alive until the next one
    with torch.cuda.device(self.device):
      self._alloc_state()
    self._pool_warned = False
    self.grow_objects = bool(grow_objects)   # check_errors() doubles the slot table before an env can fill it (_grow_objects)
    # Env(length=None): no episode may outrun the daylight table (_grow_daylight).  _step_bound >= every env's step counter.
    self._unbounded = self.cfg.length == 0
    self._step_bound = 0
    if self._unbounded and self.cfg.n_daylight < 1024:   # (crafter_extend_daylight refuses shorter tables: say so now, not deep into a run)
      raise ValueError('length=None needs a daylight table of at least 1024 steps to grow from')

  # ------------------------------------------------------------------ setup
  def _check(self, rc):
    if rc:
      raise CrafterDeviceError(_libmod.last_error(self._lib, self._handle))

  def _alloc_state(self):
    cfg = self.cfg
    self.state = {}
    for name, (shape, dt) in state.state_spec(cfg).items():
      if name == 'semantic' and not cfg.want_semantic:
        continue
      if name in state.POOL_BUFFERS and not (cfg.auto_reset and cfg.gen_period >= 0):
        continue
      self.state[name] = torch.zeros(shape, dtype=_TORCH_DTYPE[dt], device=self.device)
    rec = np.zeros(self.num_envs, abi.REC_DTYPE)
    rec['seed_lane'] = state.seed_lanes(self.seeds)
    rec['mt_pos'] = abi.MT_N
    rec['nobj'] = 1
    self.state['rec'].copy_(torch.from_numpy(rec.view(np.uint8).reshape(self.num_envs, -1)))
    self.terminal = self.state['terminal']
    self._st = self._state_ptrs()
    self._native.bind(self._st)
    n = self.num_envs
    self.obs = torch.zeros((n, cfg.size_h, cfg.size_w, 3), dtype=torch.uint8, device=self.device)
    self.reward = torch.zeros(n, dtype=torch.float32, device=self.device)
    self.done = torch.zeros(n, dtype=torch.uint8, device=self.device)
    self._rec_i32 = self.state['rec'].view(torch.int32)
    off = {name: abi.REC_DTYPE.fields[name][1] // 4 for name in abi.REC_DTYPE.names}
    self._off = off

  def _state_ptrs(self):
    """abi.StatePtrs over self.state (+ the phase-stamp buffer, if enable_phase_stamps made one)."""
    ptrs = {k: v.data_ptr() for k, v in self.state.items()}
    for name in ('semantic', 'prof') + state.POOL_BUFFERS:
      ptrs.setdefault(name, None)
    if self._prof is not None:
      ptrs['prof'] = self._prof.data_ptr()
    return abi.StatePtrs(**ptrs)

  def _mask(self, mask, check_len=False):
    """-> (contiguous uint8 device tensor or None -- for the caller to keep alive --, its pointer or None)"""
    if mask is None:
      return None, None
    mask = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
    if check_len and mask.numel() != self.num_envs:
      raise ValueError(f'mask must have {self.num_envs} elements')
    return mask, _ptr(mask)

  def _call(self, fn, *args, handle=None):
    """Every entry point that takes a stream: fn(handle, *args, the current torch stream) with the batch's device current;
    a non-zero return raises CrafterDeviceError.  handle: a _Handle other than the batch's own (render at another size)."""
    h = handle or self._native
    with torch.cuda.device(self.device):
      h.check(fn(h.ptr, *args, self._stream()))

  def _out(self, t, shape, dtype, what='out', align16=False):
    """The one check of a tensor the caller gives a kernel to write: a contiguous tensor of exactly this dtype and shape on
    the batch's device (align16: at a 16-byte aligned address).  ValueError otherwise, before anything is enqueued.  -> t"""
    if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dtype and tuple(t.shape) == tuple(shape) and
            t.is_contiguous() and not (align16 and t.data_ptr() % 16)):
      raise ValueError(f'{what} must be a contiguous{", 16-byte aligned" if align16 else ""} {dtype} tensor of shape '
                       f'{tuple(shape)} on {self.device}')
    return t

  def _step_out(self, out):
    """-> (obs, reward, done) a step writes: the batch's own, or the 16-byte aligned tensors of out = (obs or None, reward, done)."""
    if out is None:
      return self.obs, self.reward, self.done
    o, r, d = out
    like = lambda t, mine, what: self._out(t, mine.shape, mine.dtype, what, align16=True)
    return (self.obs if o is None else like(o, self.obs, 'out[0]')), like(r, self.reward, 'out[1]'), like(d, self.done, 'out[2]')

  def _rollout_out(self, T, n, out, obs):
    """-> (o, r, d) a rollout of T steps of n envs writes: u8[T,n,H,W,3] or None, f32[T,n], u8[T,n].  out None: new tensors,
    without frames if obs is false or the batch has render=False (no kernel draws, there is no frame to return).  Otherwise
    the 16-byte aligned tensors of out = (obs or None, reward, done); an obs tensor given there is written whatever `obs` says."""
    frames, scalars = ((T, n) + tuple(self.obs.shape[1:]), torch.uint8), ((T, n), torch.float32)
    if out is None:
      new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
      return (new(*frames) if obs and self.cfg.render_obs else None), new(*scalars), new((T, n), torch.uint8)
    o, r, d = out
    return (None if o is None else self._out(o, *frames, 'out[0]', align16=True),
            self._out(r, *scalars, 'out[1]', align16=True), self._out(d, (T, n), torch.uint8, 'out[2]', align16=True))

  def _actions(self, actions):
    """-> contiguous int32 device tensor"""
    if not (torch.is_tensor(actions) and actions.dtype == torch.int32 and actions.is_cuda):
      actions = torch.as_tensor(actions, device=self.device).to(torch.int32)
    return actions.contiguous()

  def __del__(self):
    try:
      for h in list(getattr(self, '_aux', {}).values()) + [getattr(self, '_native', None)]:
        if h is not None:
          h.close()
    except Exception:
      pass

  # ------------------------------------------------------------------ spaces (env.py:58-68)
  @property
  def observation_shape(self):
    return (self.cfg.size_h, self.cfg.size_w, 3)

  @property
  def num_actions(self):
    return len(self.action_names)

  @property
  def lds_bytes(self):
    return int(self._lib.crafter_lds_bytes(self._handle))

  @property
  def slot_map_derived(self):
    return bool(self._lib.crafter_slot_map_derived(self._handle))

  @property
  def step_instance(self):
    """Template instance of the step kernel this batch runs, e.g. 'crafter_step_kernel<1, 1, 1>' (maps in LDS,
    default geometry compiled in, default rules compiled in) -- the generic instances are slower."""
    k = int(self._lib.crafter_step_instance(self._handle))
    if k & 8:   # a world whose maps stay in global memory, seen through the default view (compiled in) with the default rules
      return f'crafter_step_kernel<0, 2, {k & 1}>'
    return f'crafter_step_kernel<{(k >> 2) & 1}, {(k >> 1) & 1}, {k & 1}>'

  def _stream(self):
    return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  _DAYLIGHT_MARGIN = 8

  def _grow_daylight(self, steps):
    """Env(length=None) (env.py:29): before `steps` more steps are launched, makes sure the daylight table (env.py:135-139,
    one host-evaluated value per step of an episode) reaches beyond the longest episode under way.  The bound kept
    between calls is the number of steps launched since the last look at the device; only when THAT gets near the end
    of the table (every ~100,000 calls) are the envs' step counters read back (one synchronisation) and, if an episode
    really is that long, the table doubled (crafter_extend_daylight, on every handle over this state)."""
    self._step_bound += steps
    if self._step_bound + self._DAYLIGHT_MARGIN < self.cfg.n_daylight:
      return
    self._step_bound = int(self._rec_i32[:, self._off['step']].max().item()) + steps
    need = self._step_bound + self._DAYLIGHT_MARGIN
    if need < self.cfg.n_daylight - max(1024, self.cfg.n_daylight // 8):   # (only when an episode really nears the table's end: ADVICE r4)
      return
    n = max(2 * self.cfg.n_daylight, need + tables.UNBOUNDED_DAYLIGHT)
    table = tables.daylight_table(n, head=self.tables.daylight)
    for h in [self._native] + list(self._aux.values()):
      with torch.cuda.device(self.device):
        h.check(self._lib.crafter_extend_daylight(h.ptr, table.ctypes.data_as(C.c_void_p), n))
      h.cfg.n_daylight = n
      h.tables.daylight = table
    self.cfg.n_daylight = n
    self.tables.daylight = table

  def _grow_objects(self, new_max):
    """Doubles the slot table (World._objects is an unbounded list in the reference, engine.py:50-58): synchronises, moves
    every env's table -- and its two pooled worlds' -- into larger buffers, and puts a new native handle over the state
    (`max_objects` is part of the handle's configuration and of the kernels' LDS layout: 256 slots with one-byte slot ids are
    what the default instance is compiled for, anything larger runs the generic instance).  The world pool starts afresh --
    its batches in flight belonged to the old handle: headers and request queues are cleared, an env whose next world is
    missing regenerates it inline (same generator, same (seed, episode): unobservable) and asks again."""
    new_max = int(min(new_max, 65535))
    if new_max <= self.cfg.max_objects:
      return
    torch.cuda.synchronize(self.device)
    old = self._native
    for h in self._aux.values():
      h.close()
    self._aux = {}
    cfg = abi.Config.from_buffer_copy(bytes(self.cfg))
    cfg.max_objects = new_max
    with torch.cuda.device(self.device):
      native = _Handle(self._lib, cfg, self.tables, self.device)   # (raises if one env no longer fits the LDS-resident kernels)
      for name in ('objs', 'pool_objs'):
        if name not in self.state:
          continue
        t = self.state[name]
        shape = list(t.shape)
        shape[-2] = new_max
        bigger = torch.zeros(shape, dtype=t.dtype, device=self.device)
        bigger[..., :t.shape[-2], :] = t
        self.state[name] = bigger
      for name in ('pool_hdr', 'gen_latest', 'gen_q', 'reset_q'):
        if name in self.state:
          self.state[name].zero_()
      torch.cuda.synchronize(self.device)
      self._st = self._state_ptrs()
      native.bind(self._st)
    old.close()
    was_default = self.cfg.max_objects == 256
    self._native, self._handle = native, native.ptr
    self.cfg = cfg
    self._ctor['max_objects'] = new_max
    self.objects_grown += 1
    if self._timing_on:   # handle-level settings move with the handle
      with torch.cuda.device(self.device):
        self._check(self._lib.crafter_set_timing(self._handle, 1))
    if self._levels is not None:   # ... and so does the level table
      self._enqueue_levels()
    if was_default:
      import warnings
      warnings.warn(f'crafter_amd: an environment holds more than 192 objects: the slot tables grow to {new_max} entries and the batch '
                    'leaves the compiled default instance (256 slots, one-byte slot ids) for the generic kernels, which are slower',
                    RuntimeWarning, stacklevel=3)

  # ------------------------------------------------------------------ Env API
  def reset(self, mask=None, seeds=None, episodes=None, worlds=None, world_ids=None):
    """Env.reset() (env.py:70-81) for all envs, or those with a non-zero mask byte.  Returns obs.
    seeds / episodes: reseed(seeds, episodes, mask) first, in the same call -- the named envs start episode `episodes` (1 by
    default) of `seeds`, the level a fresh crafter.Env(seed=...) shows at that reset().  episodes without seeds: the rows keep
    their seeds ("restart at episode k").
    worlds: a crafter_amd.WorldBank -- the named envs reset into AUTHORED worlds instead of generated ones: env i into world
    world_ids[i] (a host sequence or an int32 device tensor [num_envs]; None: i % len(worlds)).  Everything but the world is
    Env.reset unchanged -- the episode counter advances, the stream is RandomState(world seed) of that episode from its first
    word, counters and achievements are cleared -- and the authored world lasts this one episode: the next reset, automatic or
    not, generates episode k + 1 of the env's seed.  Host ids are checked here (ValueError); a device id outside the bank leaves
    its env as it was and sets ST_BAD_WORLD (check_errors).  The slot table grows first if the bank's longest world would fill
    three quarters of it (_grow_objects).  No host round trip: with auto_reset=False, `step(); reset(mask=done, worlds=bank,
    world_ids=ids)` keeps every env in authored worlds."""
    ids = self._world_ids(worlds, world_ids)
    if worlds is not None and self.grow_objects and 4 * worlds.max_objects > 3 * self.cfg.max_objects:   # (check_errors' own rule, ahead of the reset)
      self._grow_objects(max(2 * self.cfg.max_objects, 2 * worlds.max_objects))
    kept = self._reseed(seeds, episodes, mask) if seeds is not None or episodes is not None else None
    mask, mptr = self._mask(mask, check_len=worlds is not None)
    if worlds is None:
      self._call(self._lib.crafter_reset, mptr, _ptr(self.obs))
    else:
      t = worlds.device_tensors(self.device)
      self._call(self._lib.crafter_reset_worlds, mptr, _ptr(ids), _ptr(t['mat']), _ptr(t['objs']), _ptr(t['nobj']), _ptr(t['inv']),
                 len(worlds), int(worlds.objs.shape[1]), _ptr(self.obs))
      kept = (kept, worlds, t, ids)
    self._keep = mask if kept is None else (mask, kept)
    return self.obs

  def _world_ids(self, worlds, world_ids):
    """reset()'s checks of a WorldBank and the ids into it -> world_ids as an int32 device tensor [num_envs], or None (no bank,
    or env i into world i % len(worlds)).  Host ids are range-checked here; device ids are not read back."""
    if worlds is None:
      if world_ids is not None:
        raise ValueError('world_ids without worlds')
      return None
    _libmod.require(self._lib, 'crafter_reset_worlds', 'authored worlds')
    if tuple(worlds.area) != (int(self.cfg.W), int(self.cfg.H)):
      raise ValueError(f'the bank holds {worlds.area[0]} x {worlds.area[1]} worlds, the batch {self.cfg.W} x {self.cfg.H}')
    if worlds.inv is not None and worlds.inv.shape[1] != len(self.item_names):
      raise ValueError('the bank was made for rules with another number of items')
    if world_ids is None:
      return None
    if _on_device(world_ids):
      if world_ids.dtype != torch.int32 or tuple(world_ids.shape) != (self.num_envs,) or world_ids.device != self.device:
        raise ValueError(f'world_ids on the device must be an int32 tensor of shape [{self.num_envs}] on {self.device}')
      return world_ids.contiguous()
    a = np.asarray(world_ids.cpu() if torch.is_tensor(world_ids) else world_ids).reshape(-1)
    if a.size != self.num_envs or (a.size and not np.issubdtype(a.dtype, np.integer)):
      raise ValueError(f'world_ids must be {self.num_envs} integers')
    if a.size and (a.min() < 0 or a.max() >= len(worlds)):
      raise ValueError(f'world_ids must lie in 0 .. {len(worlds) - 1}')
    return torch.from_numpy(a.astype(np.int32)).to(self.device)

  def export_worlds(self, idx=None):
    """The current worlds of envs idx (all by default) as host arrays, in exactly the form WorldBank accepts --
    dict(mat [K, W, H], objects: per env the live objects in slot order, the player first, as (type, x, y, health, (fx, fy),
    aux), inventory [K, n_items]) -- so that `WorldBank(env, **edit(env.export_worlds()))` authors a world by editing a
    generated one.  Synchronises."""
    i, _ = self._index(np.arange(self.num_envs) if idx is None else idx, self.num_envs, 'idx')
    rows = i.long()
    rec = state.rec_view(self.state['rec'][rows].cpu().numpy())
    objs = state.objs_view(self.state['objs'][rows].cpu().numpy())
    mat = self.state['mat'][rows].cpu().numpy().reshape(-1, self.cfg.W, self.cfg.H)
    return _worlds.worlds_of(mat, objs, rec, len(self.item_names))

  # ------------------------------------------------------------------ levels (include/crafter_hip.h crafter_reseed)
  MAX_EPISODE = 2 ** 31 - 3   # the world pool asks for episode + 2

  @staticmethod
  def _host_values(x):
    """A host sequence, numpy array or CPU tensor as a list of Python values."""
    return x.tolist() if torch.is_tensor(x) or isinstance(x, np.ndarray) else list(x)

  @staticmethod
  def _lanes_arg(seeds, n=None):
    """seeds -> their 64 lane bits: the int64 / uint64 device tensor given, checked for dtype and shape ([n]; any length when
    n is None) and never read back, or the uint64 numpy array hashed from host values (n of them, when n is given)."""
    if _on_device(seeds):
      if seeds.dtype not in (torch.int64, getattr(torch, 'uint64', torch.int64)) or seeds.dim() != 1 or n not in (None, seeds.shape[0]):
        raise ValueError(f'seeds on the device must be a one-dimensional int64 / uint64 tensor{"" if n is None else f" of shape [{n}]"} '
                         '(the 64 lane bits)')
      return seeds
    seeds = BatchedEnv._host_values(seeds)
    if n is not None and len(seeds) != n:
      raise ValueError(f'len(seeds) is {len(seeds)}, the batch has {n} envs')
    return state.seed_lanes(seeds)

  @staticmethod
  def _episodes_arg(episodes, n, what):
    """episodes -> None (1 everywhere), the int32 device tensor [n] given (dtype and shape checked, never read back), or an
    int32 numpy array [n] of host values: one int for all, or n integers in 1 .. MAX_EPISODE.  `what` says in the message what
    has n entries."""
    if episodes is None:
      return None
    if _on_device(episodes):
      if episodes.dtype != torch.int32 or tuple(episodes.shape) != (n,):
        raise ValueError(f'episodes on the device must be an int32 tensor of shape [{n}]')
      return episodes
    a = np.asarray(episodes.cpu() if torch.is_tensor(episodes) else episodes)
    if a.ndim == 0:
      a = np.full(n, a[()])
    a = a.reshape(-1)
    if a.size != n:
      raise ValueError(f'len(episodes) is {a.size}, {what}')
    if a.size and not np.issubdtype(a.dtype, np.integer):
      raise ValueError('episodes must be integers')
    if a.size and (a.min() < 1 or a.max() > BatchedEnv.MAX_EPISODE):
      raise ValueError(f'episodes must lie in 1 .. {BatchedEnv.MAX_EPISODE}')
    return a.astype(np.int32)

  @staticmethod
  def _check_levels(num_envs, seeds, episodes):
    """The host side of reseed(), callable without a device: -> (lanes, episodes), each a numpy array (uint64 / int32
    [num_envs]) made of host values, the device tensor that was given, or None.  Host values are checked here and raise
    ValueError before anything is enqueued; device tensors are only checked for dtype and shape (never read back)."""
    lanes = None if seeds is None else BatchedEnv._lanes_arg(seeds, num_envs)
    return lanes, BatchedEnv._episodes_arg(episodes, num_envs, f'the batch has {num_envs} envs')

  def _level_tensors(self, lanes, eps, default_eps=None):
    """What _check_levels / _check_level_set return, as contiguous device tensors (lanes int64, eps int32).  Host arrays are
    uploaded; device tensors are passed through -- not copied -- and must be on the batch's device.  eps None: default_eps in
    every entry, or None if that is None too."""
    for t in (lanes, eps):
      if torch.is_tensor(t) and t.device != self.device:
        raise ValueError(f'level tensor on {t.device}, batch on {self.device}')
    with torch.cuda.device(self.device):
      if torch.is_tensor(lanes):
        lanes = lanes.contiguous().view(torch.int64)
      else:
        lanes = torch.from_numpy(lanes.view(np.int64)).to(self.device)
      if eps is not None:
        eps = eps.contiguous() if torch.is_tensor(eps) else torch.from_numpy(eps).to(self.device)
      elif default_eps is not None:
        eps = torch.full((lanes.numel(),), default_eps, dtype=torch.int32, device=self.device)
    return lanes, eps

  def _reseed(self, seeds, episodes, mask):
    fn = _libmod.require(self._lib, 'crafter_reseed', 'level selection')
    if seeds is not None and not _on_device(seeds):
      seeds = self._host_values(seeds)
    lanes, eps = self._check_levels(self.num_envs, seeds, episodes)
    host_seeds = seeds if isinstance(seeds, list) else None
    host_mask = None
    if mask is not None and not _on_device(mask):
      host_mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask).reshape(-1) != 0
    dmask, mptr = self._mask(mask, check_len=True)
    if lanes is None:   # episodes alone: the rows keep their lanes
      lanes = self._record_lanes()
    lanes, eps = self._level_tensors(lanes, eps)
    self._call(fn, mptr, _ptr(lanes), _ptr(eps))
    if seeds is not None:   # self.seeds: what the host knows
      if host_mask is not None:
        for i in np.nonzero(host_mask)[0]:
          self.seeds[i] = None if host_seeds is None else host_seeds[i]
      elif mask is None:
        self.seeds = [None] * self.num_envs if host_seeds is None else list(host_seeds)
      elif host_seeds is None:
        self.seeds = [None] * self.num_envs
      else:   # a mask on the device is not read back: whether a row took its new seed is only known where that changes nothing
        self.seeds = [old if old == new else None for old, new in zip(self.seeds, host_seeds)]
    self._keep = (dmask, lanes, eps)
    return self._keep

  def reseed(self, seeds, episodes=None, mask=None):
    """Chooses the level the named envs (mask: non-zero bytes; None: all) play NEXT: their next reset -- reset() or the
    automatic one -- starts episode `episodes` of `seeds`, exactly what a freshly constructed crafter.Env(seed=...) shows at
    its episodes-th reset(), and every later episode follows from there.  The episode in progress plays on unchanged; only
    its number reads episodes - 1 from now on (info['episode'], the terminal row).  Enqueued on the current stream.
    seeds: a host sequence of num_envs hashables (hashed as the reference hashes its seed: anything it accepts works), or an
    int64 / uint64 device tensor [num_envs] carrying the 64 lane bits (levels()); entries of unnamed rows are ignored.
    episodes: None (1), an int, a host sequence or an int32 device tensor [num_envs].  Host values are checked before anything
    is enqueued (ValueError: wrong length, episode outside 1 .. 2**31 - 3); device tensors are not read back -- the kernel
    takes an episode below 1 as 1.  self.seeds follows host seeds in the named rows and reads None where a device tensor was
    given (a mask on the device is not read back either: under one, every row whose seed may have changed reads None).
    With the world pool running the call brings the pool to rest first and empties the named envs' entries: each regenerates
    its next world inline once, then the pool serves it again."""
    if seeds is None:
      raise ValueError('reseed needs seeds (reset(mask, episodes=...) restarts rows at an episode of their own seeds)')
    self._reseed(seeds, episodes, mask)

  def levels(self):
    """-> (seed_lane int64 [N], episode int32 [N]): device copies of each env's seed lane and of the number of the episode it is
    in, as info() reads them.  reset(seeds=lanes, episodes=episode) on this batch, or on any batch of the same geometry,
    replays exactly those episodes from their start.
    With a level table set (set_levels) the pair is (table seed lane, table episode) of level_ids(): the levels actually
    played, and the promise still holds for reset(seeds=lanes, episodes=episode) on a batch WITHOUT a table.  As for
    level_ids(), a row is exact if its episode in progress began while this table was set."""
    if self._levels is not None:
      ids = self.level_ids().to(torch.int64)
      return self._levels['lanes'][ids], self._levels['episodes'][ids]
    return self._record_lanes(), self._rec_i32[:, self._off['episode']].clone()

  def _record_lanes(self):
    """int64 [N]: a device copy of every env's seed lane."""
    o = self._off['seed_lane']
    return self._rec_i32[:, o:o + 2].contiguous().view(torch.int64).reshape(-1)

  # ------------------------------------------------------------------ level sets (include/crafter_hip.h crafter_set_levels)
  MAX_LEVELS = state.MAX_LEVELS

  @staticmethod
  def _check_level_set(seeds, episodes, weights, key):
    """The host side of set_levels(), callable without a device: -> (lanes, episodes, cum, key).  lanes: uint64 numpy [K] or the
    device tensor given; episodes: int32 numpy [K], the device tensor given, or None (1); cum: uint32 numpy [K] or None; key:
    the 64 key bits.  Host values are checked here and raise ValueError before anything is enqueued; device tensors are only
    checked for dtype and shape."""
    lanes = BatchedEnv._lanes_arg(seeds)
    K = len(lanes)
    if not 1 <= K <= BatchedEnv.MAX_LEVELS:
      raise ValueError(f'a level table holds 1 .. {BatchedEnv.MAX_LEVELS} levels, got {K}')
    eps = BatchedEnv._episodes_arg(episodes, K, f'the table has {K} levels')
    cum = None
    if weights is not None:
      w = np.asarray(weights.cpu() if torch.is_tensor(weights) else weights).reshape(-1)
      if w.size != K:
        raise ValueError(f'len(weights) is {w.size}, the table has {K} levels')
      cum = state.levels_cum(w)
    return lanes, eps, cum, int(key) & 0xFFFFFFFFFFFFFFFF

  def _enqueue_levels(self):
    """crafter_set_levels with the table the batch keeps (None: clear)."""
    t = self._levels
    if t is None:
      self._call(self._lib.crafter_set_levels, None, None, None, 0, 0)
    else:
      self._call(self._lib.crafter_set_levels, _ptr(t['lanes']), _ptr(t['episodes']), _ptr(t['cum']), int(t['lanes'].numel()), t['key'])

  def set_levels(self, seeds, episodes=None, weights=None, key=0):
    """Sets the batch's LEVEL TABLE: K levels (seeds[j], episodes[j]), each the episode a fresh crafter.Env(seed=seeds[j]) shows
    at its episodes[j]-th reset().  While it is set, every reset -- reset(), the automatic one, from the world pool or inline --
    that takes an env into its k-th episode (k = info['episode'] of the new episode) plays level
    j = crafter_amd.levels_pick(lane, k, K, cum, key), a counter-based hash of the env's own seed lane and k: uniform over the
    table, or with probability weights[j] / sum(weights) (a level of weight 0 is not drawn).  No host round trip per finished
    env, and the world pool keeps serving.  Each env's seed and episode count keep their values and meaning (its draw lane and
    its reset count): info['episode'], the terminal row and self.seeds do not change.
    seeds: a host sequence of K hashables, hashed as the reference hashes its seed, or an int64 / uint64 device tensor [K] of
    lane bits (the first element of levels() of a batch without a table); 1 <= K <= 65536.  episodes: None (1), an int, a host
    sequence or an int32 device tensor [K].  weights: None (uniform) or K non-negative numbers, not all zero.  key: 64 bits
    that select another draw sequence over the same table.  Host values are checked before anything is enqueued (ValueError:
    wrong lengths, K > 65536, an episode outside 1 .. MAX_EPISODE, negative or all-zero weights); device tensors are not read
    back -- the kernel takes an episode below 1 as 1.  set_levels(None) clears the table: from each env's next reset on the
    batch plays the episodes of its own seeds again.
    Enqueued on the current stream; the batch keeps the table's device tensors.  Episodes in progress play on: the table takes
    effect at each env's next reset.  With the world pool running the call brings the pool to rest and empties EVERY env's
    entries (they hold worlds of the table being replaced): each env regenerates its next world inline once, then the pool
    serves it again -- a call for when the table changes, not for every step.
    With a table set, reseed() / reset(seeds=, episodes=) choose an env's position in its draw sequence, not its level:
    held-out evaluation on the same batch clears the table first.  copy_envs / save_state / load_state carry lane and episode
    count, so a copy plays the levels its source would; a store loaded under another table follows that table."""
    _libmod.require(self._lib, 'crafter_set_levels', 'level sets')
    if seeds is None:
      if episodes is not None or weights is not None:
        raise ValueError('set_levels(None) clears the table: episodes / weights need seeds')
      self._levels = None
      self._enqueue_levels()
      return
    lanes, eps, cum, key = self._check_level_set(seeds, episodes, weights, key)
    lanes, eps = self._level_tensors(lanes, eps, default_eps=1)
    if _on_device(seeds):   # the batch keeps the table: tensors of the caller's are copied
      lanes = lanes.clone()
    if _on_device(episodes):
      eps = eps.clone()
    cum_t = None if cum is None else torch.from_numpy(cum.view(np.int32)).to(self.device)   # (the 32 bits of each uint32)
    self._levels = {'lanes': lanes, 'episodes': eps, 'cum': cum_t, 'key': key, 'cum_host': cum}
    self._enqueue_levels()

  def level_ids(self, mask=None, out=None):
    """int32 [N] on the device: the index of the level-table entry of each env's episode in progress -- levels_pick(lane,
    info['episode']) under the table in force --, -1 in every row while no table is set.  Exact for an episode that began while
    this table was set (one begun under an earlier table, or before a reseed(), reads what the present table and record say).
    The exact use: after a step(), the ids of the rows with done != 0 are the levels of the episodes that just began; a
    level-replay loop keeps its own [N] tensor of them.  Read-only, no wait for the world pool.  mask: rows with a zero byte
    are left untouched.  out: a contiguous int32 device tensor [N] to write into."""
    fn = _libmod.require(self._lib, 'crafter_level_ids', 'level sets')
    if out is None:
      out = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
    else:
      self._out(out, (self.num_envs,), torch.int32)
    mask, mptr = self._mask(mask, check_len=True)
    self._call(fn, mptr, _ptr(out))
    self._keep = mask
    return out

  def step(self, actions, info=True, out=None, final=False):
    """Env.step() (env.py:83-118) for all envs.  actions: int tensor [N] on the device.
    Returns (obs u8[N,H,W,3], reward f32[N], done u8[N], info dict of device tensor views).
    With auto_reset, a finished env comes back already regenerated (its obs is the first frame
    of the next episode; done/reward still describe the finished step).
    out = (obs or None, reward, done): device tensors the kernels write instead of self.obs / self.reward /
    self.done (e.g. the send buffer of crafter_amd.dist.StepExchange); obs must be 16-byte aligned.
    final=True (auto_reset batches only; crafter_step_final): the info dict also carries, whatever `info` is, what the
    finished episodes left behind -- 'final_obs' u8[N,H,W,3], the frame the reference returns with done=True (absent with
    render=False); 'terminated' u8[N], 1 if the player died (discount == 0), 0 if the episode only ran into `length`;
    'final_local' / 'final_stats', symbolic()'s pair of the terminal state.  These are persistent device tensors of the batch,
    zero-initialised at first use; a step only writes the rows of envs it finished: rows are valid where done != 0.  Everything
    else the call returns and leaves behind is bit-identical to final=False, and the two may be mixed."""
    actions = self._actions(actions)
    obs, reward, done = self._step_out(out)
    if final:
      return self._step_final(actions, obs, reward, done, info)
    if self._unbounded:
      self._grow_daylight(1)
    self._call(self._lib.crafter_step, _ptr(actions), _ptr(obs), _ptr(reward), _ptr(done))
    self._keep = (actions, obs, reward, done)
    return obs, reward, done, (self.info() if info else {})

  def step_envs(self, idx, actions, info=True, out=None):
    """step() for the envs idx names and for no other (crafter_step_envs): a tree search steps its scratch rows, an actor loop
    the envs whose action is ready.  idx: n env indices, 1 <= n <= N, none twice; actions: n ints, actions[i] for env idx[i].
    Returns (obs, reward, done, info) as step() does -- the full [N] tensors, of which only rows idx are new; every other row,
    of the state too, is neither read nor written.  For a named env the call is exactly step(): auto-reset, pool, terminal
    row and info['semantic'] included, and the two may be mixed freely, with rollout() and the copies too.  The launch costs
    what a batch of n envs costs.
    Host indices (lists, numpy, CPU tensors) are range- and duplicate-checked here and raise ValueError before anything is
    enqueued; a device tensor is checked on the device: a bad list refuses the whole call -- no row changes -- and
    check_errors() raises (ST_BAD_COPY).  out: as for step().  An empty idx enqueues nothing."""
    fn = _libmod.require(self._lib, 'crafter_step_envs', 'step_envs')
    i, _ = self._index(idx, self.num_envs, 'idx', unique=True)
    actions = self._actions(actions).reshape(-1)
    if actions.numel() != i.numel():
      raise ValueError(f'actions has {actions.numel()} entries, idx names {i.numel()} envs')
    if i.numel() > self.num_envs:
      raise ValueError(f'idx names {i.numel()} envs, the batch has {self.num_envs}')
    obs, reward, done = self._step_out(out)
    if i.numel():
      if self._unbounded:
        self._grow_daylight(1)
      self._call(fn, _ptr(i), int(i.numel()), _ptr(actions), _ptr(obs), _ptr(reward), _ptr(done))
      self._keep = (i, actions, obs, reward, done)
    return obs, reward, done, (self.info() if info else {})

  def final_buffers(self):
    """The persistent device tensors step(final=True) writes and returns in its info dict: {'final_obs' (absent with
    render=False), 'terminated', 'final_local', 'final_stats'}; allocated at first use, zero-initialised."""
    if self._final is None:
      ls, ss = self.symbolic_shape
      n = self.num_envs
      with torch.cuda.device(self.device):
        f = {'terminated': torch.zeros(n, dtype=torch.uint8, device=self.device),
             'final_local': torch.zeros((n,) + ls, dtype=torch.uint8, device=self.device),
             'final_stats': torch.zeros((n,) + ss, dtype=torch.float32, device=self.device)}
        if self.cfg.render_obs:
          f['final_obs'] = torch.zeros_like(self.obs)
      self._final = f
    return self._final

  def _step_final(self, actions, obs, reward, done, info):
    if not self.cfg.auto_reset:
      raise ValueError('step(final=True) needs auto_reset=True: without it obs already is the finished episode\'s last frame')
    fn = _libmod.require(self._lib, 'crafter_step_final', 'step(final=True)')
    f = self.final_buffers()
    if self._unbounded:
      self._grow_daylight(1)
    self._call(fn, _ptr(actions), _ptr(obs), _ptr(reward), _ptr(done), _ptr(f.get('final_obs')), _ptr(f['terminated']),
               _ptr(f['final_local']), _ptr(f['final_stats']))
    self._keep = (actions, obs, reward, done)
    out = self.info() if info else {}
    out.update(f)
    return obs, reward, done, out

  def rollout(self, actions, out=None, obs=True):
    """T steps in one call for policies that choose their actions without looking at the observations (random,
    scripted, action repeat; run_random.py:36-44 is such a loop): actions int32 [T, N] on the device.  Returns
    (obs u8[T,N,H,W,3] or None, reward f32[T,N], done u8[T,N]) -- bit-identical to T calls of step(), faster because an env
    starts its step t + 1 without waiting for every other env's step t (crafter_step_n).  out = (obs or None, reward,
    done): tensors of those shapes to write into.  self.obs / self.reward / self.done are NOT updated; the state is."""
    actions = self._actions(actions)
    if actions.dim() != 2 or actions.shape[1] != self.num_envs or actions.shape[0] < 1:
      raise ValueError(f'actions must have shape [T, {self.num_envs}]')
    T = int(actions.shape[0])
    o, r, d = self._rollout_out(T, self.num_envs, out, obs)   # (render=False: no frames; step() hands out zeros)
    if self._unbounded:
      self._grow_daylight(T)
    self._call(self._lib.crafter_step_n, T, _ptr(actions), _ptr(o), _ptr(r), _ptr(d))
    self._keep = (actions, o, r, d)
    return o, r, d

  def rollout_envs(self, idx, actions, out=None, obs=True):
    """rollout() for the envs idx names and for no other, with compact outputs (crafter_step_n_envs): the playouts of a tree
    search or a random-shooting planner over the scratch rows of a large batch, an action repeat of a few envs.  idx: n env
    indices, 1 <= n <= N, none twice, any order; actions: int32 [T, n] ([n] when T == 1), actions[t, i] for env idx[i] at its
    step t.  Returns (obs u8[T,n,H,W,3] or None, reward f32[T,n], done u8[T,n]): row i belongs to env idx[i].  For a named env
    the call is exactly T calls of step_envs() that name it -- auto-reset, pool, terminal row and info['semantic'] included --
    in one launch per stretch, its state resident in LDS over the stretch; every other row, of the state too, is neither read
    nor written.  self.obs / self.reward / self.done are NOT updated; the state is.
    idx is checked as for step_envs(): host indices raise ValueError before anything is enqueued, a device tensor is checked on
    the device -- a bad list refuses the whole call, no state row and no output byte changes, and check_errors() raises
    (ST_BAD_COPY).  out = (obs or None, reward, done): tensors of those shapes to write into.  obs=False, or a batch with
    render=False: no frames.  An empty idx enqueues nothing."""
    fn = _libmod.require(self._lib, 'crafter_step_n_envs', 'rollout_envs')
    i, _ = self._index(idx, self.num_envs, 'idx', unique=True)
    n = int(i.numel())
    if n > self.num_envs:
      raise ValueError(f'idx names {n} envs, the batch has {self.num_envs}')
    actions = self._actions(actions)
    if actions.dim() == 1:
      actions = actions.reshape(1, -1)
    if actions.dim() != 2 or actions.shape[1] != n or actions.shape[0] < 1:
      raise ValueError(f'actions must have shape [T, {n}] with T >= 1 (idx names {n} envs)')
    T = int(actions.shape[0])
    o, r, d = self._rollout_out(T, n, out, obs)
    if n:
      if self._unbounded:
        self._grow_daylight(T)
      self._call(fn, _ptr(i), n, T, _ptr(actions), _ptr(o), _ptr(r), _ptr(d))
      self._keep = (i, actions, o, r, d)
    return o, r, d

  # ------------------------------------------------------------------ edits in place (include/crafter_hip_edit.h)
  def edit(self, idx, ops):
    """Edits the envs idx names in place, between two steps (crafter_edit_envs): cells, objects, the inventory, the player's
    counters and the clock, with every derived table -- slot map, census, chunk order -- following as in a step.  idx: n env
    indices, none twice.  ops: one tape (a list of crafter_amd.edits ops: set_cell, add, remove, move, set_object, set_item,
    set_player, set_clock) applied to every named env, or a list of n tapes, or an int32 device tensor [n, L, 8] in the
    encoding of edits.encode() (padded with NOP), which is not read back: a loop can build its tapes with torch and never leave
    the device.  Each op means what the reference statement it is named after means between two Env.step calls; an edit draws
    nothing from the env's RNG, leaves obs / reward / done / info['semantic'] as they are (render() shows an edit at once) and
    neither reads nor writes any other row; the edited episode ends and auto-resets like any other.
    Host tapes are checked by edits.encode() and raise ValueError before anything is enqueued; what only the state can tell
    (an occupied cell, no object where one is meant) and everything in a device tensor is checked on the device: such an op is
    skipped or repaired, the tape's other ops are applied and check_errors() raises (ST_BAD_EDIT).  idx is checked as for
    step_envs().  An empty idx enqueues nothing."""
    from . import edits as _edits
    fn = _libmod.require(self._lib, 'crafter_edit_envs', 'edit()')
    i, _ = self._index(idx, self.num_envs, 'idx', unique=True)
    n = int(i.numel())
    if n > self.num_envs:
      raise ValueError(f'idx names {n} envs, the batch has {self.num_envs}')
    if _on_device(ops):
      if ops.device != self.device:
        raise ValueError(f'ops on {ops.device}, batch on {self.device}')
      if ops.dtype != torch.int32 or ops.dim() != 3 or ops.shape[0] != n or ops.shape[1] < 1 or ops.shape[2] != _edits.WORDS:
        raise ValueError(f'a device tape is int32 [{n}, L, {_edits.WORDS}] with L >= 1 (idx names {n} envs)')
      tape = ops.contiguous()
      if tape.data_ptr() % 16:
        tape = tape.clone()
    else:
      tape = torch.from_numpy(_edits.encode(self, ops, n)).to(self.device)
    if n:
      self._call(fn, _ptr(i), n, _ptr(tape), int(tape.shape[1]))
      self._keep = (i, tape)
      if self._unbounded:   # a clock op may have set a step beyond any this batch ran: the next _grow_daylight reads the counters
        self._step_bound = self.cfg.n_daylight

  def _render_handle(self, size):
    """A second handle with another frame size over the SAME state buffers: Env.render(size)
    (env.py:120-130; the reference's VideoRecorder asks for 512x512, recorder.py:92)."""
    size = tuple(int(v) for v in (size if hasattr(size, '__len__') else (size, size)))
    if size == (self.cfg.size_w, self.cfg.size_h):
      return self._native
    if size not in self._aux:
      k = self._ctor
      cfg, geo = tables.make_config(self.num_envs, self.rules, k['area'], k['view'], size, k['reward'], k['length'],
                                    max_objects=k['max_objects'], auto_reset=False, want_semantic=False,
                                    render_obs=True, n_daylight=self.cfg.n_daylight)
      cfg.gen_period = -1
      h = _Handle(self._lib, cfg, tables.HostTables(self.rules, self._textures, cfg, geo), self.device)
      h.bind(self._st)
      self._aux[size] = h
    return self._aux[size]

  def render(self, size=None, mask=None, out=None):
    """Env.render(size) (env.py:120-130) for all / masked envs; like the reference it re-draws the frame and
    consumes the night noise from each env's RNG again.  Returns uint8 [N, size[1], size[0], 3]."""
    h = self._native if size is None else self._render_handle(size)
    shape = (self.num_envs, h.cfg.size_h, h.cfg.size_w, 3)
    out = torch.zeros(shape, dtype=torch.uint8, device=self.device) if out is None else out
    mask, mptr = self._mask(mask)
    self._call(self._lib.crafter_render, mptr, _ptr(out), handle=h)
    self._keep = mask
    return out

  # ------------------------------------------------------------------ symbolic observation (include/crafter_hip.h crafter_symbolic)
  _OBJECT_CLASSES = ('player', 'cow', 'zombie', 'skeleton', 'arrow', 'plant')   # env.py:47-49, crafter_hip_types.h CRAFTER_T_*

  @property
  def symbolic_shape(self):
    """((2, gw, gh), (n_items + 4,)): the per-env shapes of symbolic()'s pair."""
    return (2, int(self.cfg.local_gw), int(self.cfg.local_gh)), (len(self.item_names) + 4,)

  @property
  def symbolic_names(self):
    """{'classes': names indexed by the plane-0 id ('none', the materials, then player ... plant), 'stats': the column names
    of stats}."""
    return {'classes': ['none'] + list(self.rules['materials']) + list(self._OBJECT_CLASSES),
            'stats': list(self.item_names) + ['facing_x', 'facing_y', 'sleeping', 'daylight']}

  def symbolic(self, mask=None, out=None):
    """The state self.obs depicts, as numbers: (local u8 [N, 2, gw, gh], stats f32 [N, n_items + 4]) on the device.
    local[e, 0, x, y] is what info['semantic'] holds at world cell player.pos + (x, y) - (gw // 2, gh // 2) -- the cell the
    frame shows there (engine.py:155-187) -- and 0 outside the world; local[e, 1, x, y] is the sprite variant of the object on
    it (player 1 left, 2 right, 3 up, 4 down, 5 sleeping; arrow 1 .. 4; ripe plant 1; else 0).  stats: the inventory in
    item_names order, facing x / y, sleeping, daylight (symbolic_names).  After a step() that auto-reset an env the pair
    describes the new episode's first state, after a rollout() the state behind its last step.  Read-only: unlike render()
    it draws nothing from the envs' RNG; works whatever `render` and `semantic` were.  mask: rows with a zero byte are left
    untouched.  out = (local, stats): contiguous device tensors of exactly those dtypes and shapes to write into."""
    ls, ss = self.symbolic_shape
    shapes = ((self.num_envs,) + ls, torch.uint8), ((self.num_envs,) + ss, torch.float32)
    if out is None:
      out = tuple(torch.zeros(shape, dtype=dt, device=self.device) for shape, dt in shapes)
    else:
      if len(out) != 2:
        raise ValueError('out must be a pair (local, stats)')
      for k, (t, (shape, dt)) in enumerate(zip(out, shapes)):
        self._out(t, shape, dt, f'out[{k}]')
    mask, mptr = self._mask(mask, check_len=True)
    local, stats = out
    self._call(self._lib.crafter_symbolic, mptr, _ptr(local), _ptr(stats))
    self._keep = mask
    return local, stats

  # ------------------------------------------------------------------ legal-action mask (include/crafter_hip.h crafter_legal_actions)
  def legal_actions(self, mask=None, out=None):
    """uint8 [N, num_actions] on the device, in action_names order: legal[e, a] = 1 iff Player.update (objects.py:99-131), run
    on env e's current state with action a, passes every guard of that action's branch.  With target = pos + facing and
    awake = not (sleeping and energy < max): noop always; move_* iff awake and the destination is inside the world, free of
    objects and walkable for the player (iff the position would change: a blocked move still turns and is not legal); do iff
    awake and target holds a zombie, skeleton, cow or ripe plant, or no object and water or a material whose collect rule's
    `require` the inventory holds; sleep iff not sleeping and energy < max; place_* iff awake, target free of objects, its
    material in `where` and `uses` in the inventory; make_* iff awake, every `nearby` material in the 3 x 3 window (numpy's
    slices: empty at x == 0 or y == 0) and `uses` in the inventory.  For every action but a move, 0 means the step does what
    noop does.  The guards are this batch's `rules`.
    After a step() that auto-reset an env the row describes the new episode's first state, after a rollout() the state behind
    its last step.  Read-only: no draw from the envs' RNG, no byte of state changes.  mask: rows with a zero byte are left
    untouched.  out: a contiguous uint8 device tensor of exactly that shape to write into."""
    shape = (self.num_envs, self.num_actions)
    if out is None:
      out = torch.zeros(shape, dtype=torch.uint8, device=self.device)
    else:
      self._out(out, shape, torch.uint8)
    mask, mptr = self._mask(mask, check_len=True)
    self._call(self._lib.crafter_legal_actions, mptr, _ptr(out))
    self._keep = mask
    return out

  # ------------------------------------------------------------------ state fingerprints (include/crafter_hip_fingerprint.h)
  def _fingerprint(self, parts, mask, key, part_hash):
    fn = _libmod.require(self._lib, 'crafter_fingerprint', 'fingerprint()')
    mask, mptr = self._mask(mask, check_len=True)
    self._call(fn, mptr, int(parts) & 0xFFFFFFFF, _ptr(key), _ptr(part_hash))
    self._keep = mask

  def fingerprint(self, parts=abi.FP_DYNAMICS, mask=None, out=None):
    """int64 [N] on the device: each env's 64-bit state key over the parts of the bit mask `parts` (crafter_amd.FP_MAP, FP_OBJECTS,
    FP_PLAYER, FP_CLOCK, FP_RNG, FP_CHUNKS, FP_IDENT; FP_VISIBLE = map | objects | player, FP_DYNAMICS = all but FP_IDENT,
    FP_ALL); the tensor carries the 64 bits (`& 0xFFFFFFFFFFFFFFFF` on a Python int gives the unsigned value
    crafter_amd.fingerprint_host computes).  Two rows have equal keys iff -- up to a 64-bit collision; the hash is not
    cryptographic -- their canonical states (snapshot(i)) agree on those parts: free slot-table records, holes in the table,
    derived maps, status bits, the last step's outputs and the world pool do not enter.  Two rows with equal FP_DYNAMICS keys
    produce identical outputs under any common action sequence until the episode ends (FP_IDENT adds which level comes next).
    After a step() that auto-reset an env the key is the new episode's first state's.  Read-only: no draw from the envs' RNG, no
    byte of state changes.  mask: rows with a zero byte are left untouched.  out: a contiguous int64 device tensor of shape
    [N] to write into.  A `parts` of 0 or with a bit above FP_IDENT raises CrafterDeviceError."""
    if out is None:
      out = torch.zeros((self.num_envs,), dtype=torch.int64, device=self.device)
    else:
      self._out(out, (self.num_envs,), torch.int64)
    self._fingerprint(parts, mask, out, None)
    return out

  def fingerprint_parts(self, mask=None, out=None):
    """int64 [N, FP_PARTS] on the device: the hash of each part by itself, column p for bit p (map, objects, player, clock, rng,
    chunks, ident) -- which part of two states differs.  mask, out: as fingerprint()."""
    shape = (self.num_envs, abi.FP_PARTS)
    if out is None:
      out = torch.zeros(shape, dtype=torch.int64, device=self.device)
    else:
      self._out(out, shape, torch.int64)
    self._fingerprint(0, mask, None, out)
    return out

  # ------------------------------------------------------------------ the audit of the rows (include/crafter_hip_audit.h)
  def audit(self, mask=None, out=None):
    """(flags int32 [N], detail int32 [N, 4]) on the device: every table the step kernels derive from mat / objs / rec and then
    trust -- the cell -> slot map where it is state, the five census columns per chunk, chunk_order / chunk_seen / nchunks_seen --
    recounted from those three, one launch for the batch.  flags[e] = 0: row e is a row; else bit b names abi.AUDIT_NAMES[b]
    (NOT_RESET, REC, PLAYER, OBJECT, CELL, SLOTMAP, MATERIAL, SPACE, CREATURES, CHUNKS, CHUNK_MISSING; crafter_hip_audit.h says
    when each holds) and detail[e] = (bit, index, found, expected) of the lowest failing bit at its lowest offending slot, cell
    x * H + y, census word chunk * 5 + column or chunk_order position (-1 where a value means nothing; four -1 for a consistent
    row).  For rows written from outside -- edit tapes, load_state, WorldBank, copy_envs, pokes into `state` -- and for soaks:
    check_errors() only reports what a kernel happened to notice.  Safe on garbage: nothing read from a row is used as an index
    before it is bounded.  Read-only: it writes its outputs only, draws nothing from the RNG, sets no status bit, does not look
    at the world pool.  Does not synchronise.  mask: rows with a zero byte are left untouched.  out = (flags, detail): contiguous
    int32 device tensors of exactly those shapes to write into.  crafter_amd.audit_host is the numpy mirror."""
    fn = _libmod.require(self._lib, 'crafter_audit', 'audit()')
    shapes = (self.num_envs,), (self.num_envs, 4)
    if out is None:
      out = torch.zeros(shapes[0], dtype=torch.int32, device=self.device), torch.full(shapes[1], -1, dtype=torch.int32, device=self.device)
    else:
      if len(out) != 2:
        raise ValueError('out must be a pair (flags, detail)')
      for k, (t, shape) in enumerate(zip(out, shapes)):
        self._out(t, shape, torch.int32, f'out[{k}]')
    mask, mptr = self._mask(mask, check_len=True)
    flags, detail = out
    self._call(fn, mptr, _ptr(flags), _ptr(detail))
    self._keep = mask
    return flags, detail

  def assert_consistent(self, mask=None, limit=4):
    """audit(mask), read back (synchronises): raises CrafterDeviceError naming the first `limit` inconsistent rows, the
    invariants each fails and the detail of its lowest one."""
    flags, detail = self.audit(mask)   # (rows the mask leaves out keep the fresh tensors' 0)
    bad = torch.nonzero(flags).flatten()
    if not bad.numel():
      return
    rows = []
    for i in bad[:limit].tolist():
      bits, (bit, index, found, expected) = int(flags[i]), detail[i].tolist()
      names = [name for b, name in enumerate(abi.AUDIT_NAMES) if bits >> b & 1]
      where = f' at chunk {index // 5} column {index % 5}' if bit in (7, 8) else ''
      rows.append(f'env {i}: {", ".join(names)} ({abi.AUDIT_NAMES[bit]}: index {index}{where}, found {found}, expected {expected})')
    raise CrafterDeviceError(f'{bad.numel()} inconsistent rows -- ' + '; '.join(rows))

  # ------------------------------------------------------------------ navigation queries (include/crafter_hip_navigate.h)
  @staticmethod
  def _class_set(names, entry, what):
    """One entry of `targets` / `passable` -- a name of `names`, an id, or a list of either -- as a bit set over the ids
    1 .. len(names) - 1 (id 0, 'none', is no cell's class).  ValueError for anything else, and for an empty set."""
    items = list(entry) if isinstance(entry, (list, tuple, set, frozenset)) else [entry]
    bits = 0
    for item in items:
      if isinstance(item, str):
        if item not in names[1:]:
          raise ValueError(f'{what}: unknown name {item!r} (one of {names[1:]})')
        c = names.index(item, 1)
      elif isinstance(item, (int, np.integer)) and not isinstance(item, bool):
        c = int(item)
        if not 1 <= c < len(names):
          raise ValueError(f'{what}: id {c} outside 1 .. {len(names) - 1}')
      else:
        raise ValueError(f'{what}: {item!r} is neither a name nor an id')
      bits |= 1 << c
    if not bits:
      raise ValueError(f'{what}: an empty set')
    return bits

  @staticmethod
  def _check_targets(class_names, n_materials, walkable, targets, passable=None):
    """The host side of navigate(), callable without a device: -> (the K target class sets, the passable material set) as
    ints.  class_names: symbolic_names['classes']; walkable: the rules' walkable list, the default of `passable`.  ValueError
    before anything is enqueued: K outside 1 .. NAV_MAX_TARGETS, an unknown name, 'none' / id 0, an id beyond the classes
    (the materials, for `passable`), an empty set, more than 31 classes."""
    names = list(class_names)
    if len(names) > 31:
      raise ValueError(f'navigate() holds a class set in 32 bits: {len(names)} classes are too many')
    if isinstance(targets, (str, int, np.integer)) or not hasattr(targets, '__len__'):
      raise ValueError('targets must be a sequence of names, ids or lists of them (one entry per query)')
    if not 1 <= len(targets) <= abi.NAV_MAX_TARGETS:
      raise ValueError(f'targets must have 1 .. {abi.NAV_MAX_TARGETS} entries, not {len(targets)}')
    sets = [BatchedEnv._class_set(names, t, f'targets[{k}]') for k, t in enumerate(targets)]
    walk = BatchedEnv._class_set(names[:n_materials + 1], list(walkable) if passable is None else passable, 'passable')
    return sets, walk

  def class_mask(self, names_or_ids):
    """The 32-bit class set navigate() takes for a name of symbolic_names['classes'], a class id, or a list of either."""
    return self._class_set(self.symbolic_names['classes'], names_or_ids, 'class_mask')

  def navigate(self, targets, passable=None, mask=None, out=None):
    """(dist int32 [N, K], first int32 [N, K], facing uint8 [N, K]) on the device: for each env and each of the K entries of
    `targets`, how far on foot the nearest cell of that kind is and which move comes first.  An entry is a class name of
    symbolic_names['classes'] ('tree', 'water', 'cow', ...), a class id, or a list of either (a set: ['coal', 'iron']);
    passable: names or ids of the materials one walks on (default: the rules' `walkable` -- grass, sand, path --, what a plain
    object walks on, objects.py:44-47; the player's own set adds 'lava').  A cell counts as a target by what info['semantic']
    shows on it -- the object standing there, else the material --, the player's own cell never; one walks over passable cells
    that hold no object.  dist: the number of move actions after which the player faces the target (or stands on it, if it is
    passable and free) provided nothing else moves, -1 if no walk exists; always >= 1 otherwise.  first: the index in
    action_names of the first move of a shortest walk -- of left, right, up, down the first that shortens it --, -1 where dist
    is -1.  facing: 1 iff the cell in front of the player is a target ("`do` now").  The query ignores sleeping, damage and
    what creatures will do next.  After a step() that auto-reset an env the row describes the new episode's first state, after
    a rollout() the state behind its last step.  Read-only: no draw from the envs' RNG, no byte of state changes.  mask: rows
    with a zero byte are left untouched.  out = (dist, first, facing): contiguous device tensors of exactly those dtypes and
    shapes to write into.  Bad targets raise ValueError before anything is enqueued."""
    fn = _libmod.require(self._lib, 'crafter_navigate', 'navigate()')
    sets, walk = self._check_targets(self.symbolic_names['classes'], len(self.rules['materials']), self.rules['walkable'], targets, passable)
    K = len(sets)
    dtypes = (torch.int32, torch.int32, torch.uint8)
    if out is None:
      out = tuple(torch.zeros((self.num_envs, K), dtype=dt, device=self.device) for dt in dtypes)
    else:
      if len(out) != 3:
        raise ValueError('out must be a triple (dist, first, facing)')
      for k, (t, dt) in enumerate(zip(out, dtypes)):
        self._out(t, (self.num_envs, K), dt, f'out[{k}]')
    mask, mptr = self._mask(mask, check_len=True)
    host = (C.c_uint32 * K)(*sets)   # read before the call returns
    dist, first, facing = out
    self._call(fn, mptr, C.cast(host, C.c_void_p), K, walk, _ptr(dist), _ptr(first), _ptr(facing))
    self._keep = mask
    return dist, first, facing

  # ------------------------------------------------------------------ nearby queries (include/crafter_hip_nearby.h)
  @staticmethod
  def _check_nearby(class_names, n_materials, area, max_objects, distance=None, k=16, classes=None, numpy_slices=False):
    """The host side of nearby(), callable without a device: -> (distance, flags, the class set) as ints.  class_names:
    symbolic_names['classes'].  ValueError before anything is enqueued: k outside 0 .. NEARBY_MAX_ENTS, a distance that is no
    integer, numpy_slices with the whole world, an unknown name, a class that is no object class, more than 31 classes, and
    with k > 0 a world with a side above NEARBY_MAX_SIDE or more slots than the kernel's key table holds."""
    names = list(class_names)
    if len(names) > 31:
      raise ValueError(f'nearby() holds a class set in 32 bits: {len(names)} classes are too many')
    integer = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not integer(k) or not 0 <= k <= abi.NEARBY_MAX_ENTS:
      raise ValueError(f'k must be an integer in 0 .. {abi.NEARBY_MAX_ENTS}, not {k!r}')
    if distance is not None and not integer(distance):
      raise ValueError(f'distance must be None (the whole world) or an integer, not {distance!r}')
    d = -1 if distance is None or distance < 0 else int(min(distance, 1 << 20))
    if numpy_slices and d < 0:
      raise ValueError('numpy_slices needs a distance >= 0: the reference has no slice for the whole world')
    objects = 0x3F << (n_materials + 1)
    if classes is None:
      bits = objects & ~(1 << (n_materials + abi.T_PLAYER))
    elif isinstance(classes, (list, tuple, set, frozenset)) and not len(classes):
      bits = 0
    else:
      bits = BatchedEnv._class_set(names, classes, 'classes')
    if bits & ~objects:
      raise ValueError(f'classes: only the object classes {names[n_materials + 1:]} can be listed')
    if k > 0 and (max(area) > abi.NEARBY_MAX_SIDE or (40 + 32 + max_objects) * 4 > 64 * 1024):
      raise ValueError(f'nearby(k > 0) serves worlds of at most {abi.NEARBY_MAX_SIDE} cells a side and about 16000 slots; k=0 gives the counts')
    return d, abi.NEARBY_NUMPY if numpy_slices else abi.NEARBY_CLIP, bits

  def nearby(self, distance=None, k=16, classes=None, numpy_slices=False, mask=None, out=None):
    """(counts int32 [N, C], ents int16 [N, k, 6], n int32 [N]) on the device: what World.nearby(player.pos, distance) and
    World.count say about every env (engine.py:95-110), and the k nearest objects.  The window is the square of cells within
    `distance` of the player on both axes, clipped to the world; None (or a negative distance): the whole world.
    numpy_slices=True: exactly the cells the reference's own `_mat_map[x - d: x + d + 1, y - d: y + d + 1]` selects -- EMPTY one
    or two cells from the west or north border, which is why the reference cannot craft there.  counts, in the class ids of
    symbolic_names['classes'] (C = len of it): [e, 0] the cells of the window, [e, m] the window cells of material m whatever
    stands on them, [e, n_materials + t] the live objects of type t in the window, the player included.  ents[e, j], j < min(n[e],
    k): the j-th nearest object whose class is in `classes` -- names, ids or a list of them as navigate() takes; default every
    object class but the player; [] none -- in ascending dx^2 + dy^2, then dx, then dy, as abi.NEARBY_COLUMNS = (class id, dx, dy,
    health, facing code, aux): the facing code is symbolic()'s plane-1 variant (arrow 1 .. 4, ripe plant 1, else 0), aux is
    saturated to int16.  n[e] counts every object that qualified and may exceed k; rows from min(n, k) on are zeros.  k = 0 skips
    the list (ents has no rows, n is zeros).  A row never reset gives zeros.  After a step() that auto-reset an env the row
    describes the new episode's first state, after a rollout() the state behind its last step.  Read-only: no draw from the
    envs' RNG, no byte of state changes, no wait for the world pool.  Does not synchronise.  mask: rows with a zero byte are left
    untouched.  out = (counts, ents, n): contiguous device tensors of exactly those dtypes and shapes to write into.  Bad
    arguments raise ValueError before anything is enqueued.  crafter_amd.nearby_host is the numpy mirror."""
    fn = _libmod.require(self._lib, 'crafter_nearby', 'nearby()')
    names = self.symbolic_names['classes']
    d, flags, bits = self._check_nearby(names, len(self.rules['materials']), (self.cfg.W, self.cfg.H), self.cfg.max_objects,
                                        distance, k, classes, numpy_slices)
    shapes = ((self.num_envs, len(names)), torch.int32), ((self.num_envs, k, abi.NEARBY_ROW), torch.int16), ((self.num_envs,), torch.int32)
    if out is None:
      out = tuple(torch.zeros(shape, dtype=dt, device=self.device) for shape, dt in shapes)
    else:
      if len(out) != 3:
        raise ValueError('out must be a triple (counts, ents, n)')
      for j, (t, (shape, dt)) in enumerate(zip(out, shapes)):
        self._out(t, shape, dt, f'out[{j}]')
    mask, mptr = self._mask(mask, check_len=True)
    counts, ents, n = out
    self._call(fn, mptr, d, flags, bits, k, _ptr(counts), _ptr(ents) if k else None, _ptr(n) if k else None)
    self._keep = mask
    return counts, ents, n

  def count(self, material):
    """World.count(material) of every env (engine.py:109-110): int32 [N] on the device, a view of one whole-world nearby(k=0)
    call.  material: a name of rules['materials'] or its id."""
    names = ['none'] + list(self.rules['materials'])
    bits = self._class_set(names, material, 'material')
    if bits & (bits - 1):
      raise ValueError('material: one name or id')
    return self.nearby(None, k=0)[0][:, bits.bit_length() - 1]

  def info(self):
    """Device-tensor views of what the reference puts into ``info`` (env.py:108-115)."""
    o, r = self._off, self._rec_i32
    ni, na = len(self.item_names), len(self.achievement_names)
    objs = self.state['objs']
    out = {
        'inventory': r[:, o['inv']: o['inv'] + ni],
        'achievements': r[:, o['ach']: o['ach'] + na],
        'discount': 1.0 - r[:, o['dead']].to(torch.float32),
        'player_pos': objs[:, 1, 4:8].view(torch.int16).to(torch.int32),
        'step': r[:, o['step']],
        'episode': r[:, o['episode']],
    }
    if self.cfg.want_semantic:
      out['semantic'] = self.state['semantic'].view(self.num_envs, self.cfg.W, self.cfg.H)
    return out

  # ------------------------------------------------------------------ copies of envs
  @staticmethod
  def _host_index(idx, rows, what, unique=False):
    """Host indices (a list, a numpy array, a CPU tensor), callable without a device: -> int64 numpy, flat.  ValueError unless
    they are integers in 0 .. rows - 1 and, with unique, name no row twice."""
    a = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1)
    if a.size and not np.issubdtype(a.dtype, np.integer):
      raise ValueError(f'{what}: indices must be integers')
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= rows):
      raise ValueError(f'{what}: index out of range 0 .. {rows - 1}')
    if unique and len(np.unique(a)) != len(a):
      raise ValueError(f'{what} names an env twice')
    return a

  def _index(self, idx, rows, what, unique=False):
    """-> (contiguous device int32 tensor, the host values or None).  Host indices are checked here (_host_index) and raise
    ValueError before anything is enqueued; device tensors are not read back: the library checks them on the device (ST_BAD_COPY)."""
    if _on_device(idx):
      if idx.device != self.device:
        raise ValueError(f'{what}: index tensor on {idx.device}, batch on {self.device}')
      return idx.reshape(-1).to(torch.int32).contiguous(), None
    a = self._host_index(idx, rows, what, unique)
    return torch.from_numpy(a.astype(np.int32)).to(self.device), a

  def _geometry(self):
    return dict(area=(int(self.cfg.W), int(self.cfg.H)), view=tuple(int(v) for v in self._ctor['view']),
                size=(int(self.cfg.size_w), int(self.cfg.size_h)), length=int(self.cfg.length),
                rules=hashlib.sha256(self.tables.rules_bytes().tobytes()).hexdigest()[:16], semantic=bool(self.cfg.want_semantic),
                slot_map_derived=self.slot_map_derived)

  def copy_envs(self, src, dst):
    """Env dst[i] becomes an exact copy of env src[i] (what copy.deepcopy of the reference's crafter.Env carries, and the obs /
    reward / done rows), as it stands after every call enqueued so far; stepped on, it lives the future the source would have,
    later episodes included.  Enqueued on the current stream.  A destination named twice or also named as a source is refused:
    host indices raise ValueError, device indices refuse the whole call on the device (check_errors: ST_BAD_COPY)."""
    s, hs = self._index(src, self.num_envs, 'src')
    d, hd = self._index(dst, self.num_envs, 'dst', unique=True)
    if s.numel() != d.numel():
      raise ValueError('src and dst must have the same length')
    if hs is not None and hd is not None and np.intersect1d(hs, hd).size:
      raise ValueError('an env is both a source and a destination')
    self._call(self._lib.crafter_copy_envs, _ptr(s), _ptr(d), int(s.numel()), _ptr(self.obs), _ptr(self.reward), _ptr(self.done))
    self._keep = (s, d)

  def save_state(self, idx=None):
    """-> EnvStore holding copies of envs idx (all by default) as they stand after every call enqueued so far."""
    i, _ = self._index(np.arange(self.num_envs) if idx is None else idx, self.num_envs, 'idx')
    rows = int(i.numel())
    spec = state.store_spec(self.cfg, rows, self.slot_map_derived)
    store = EnvStore({k: torch.zeros(shape, dtype=_TORCH_DTYPE[dt], device=self.device) for k, (shape, dt) in spec.items()},
                     self._geometry(), i)
    t = store.tensors
    ptrs = store._ptrs()
    self._call(self._lib.crafter_save_envs, _ptr(i), rows, _ptr(self.obs), _ptr(self.reward), _ptr(self.done), C.byref(ptrs), rows,
               store.max_objects, _ptr(t['obs']), _ptr(t['reward']), _ptr(t['done']))
    self._keep = i
    return store

  def load_state(self, store, idx=None, rows=None):
    """Writes store rows `rows` (all by default) into envs idx (by default the envs the store was taken from), which then go on
    exactly as the saved envs would have.  The store must come from a batch of the same area, view, size, rules and length on
    this device; a store with a wider slot table grows this batch first (_grow_objects)."""
    mine, theirs = self._geometry(), store.geometry
    for key in ('area', 'view', 'size', 'length', 'rules', 'slot_map_derived'):
      if mine[key] != theirs[key]:
        raise ValueError(f'load_state: the store was taken with another {key} than this batch has')
    if mine['semantic'] and not theirs['semantic']:
      raise ValueError('load_state: this batch keeps info["semantic"], the store was taken without it')
    if store.device != self.device:
      raise ValueError(f'load_state: the store is on {store.device}, the batch on {self.device} (EnvStore.to)')
    if store.max_objects > self.cfg.max_objects:
      self._grow_objects(store.max_objects)
    d, _ = self._index(store.idx if idx is None else idx, self.num_envs, 'idx', unique=True)
    r = None
    if rows is not None:
      r, _ = self._index(rows, len(store), 'rows')
      if r.numel() != d.numel():
        raise ValueError('rows and idx must have the same length')
    elif d.numel() > len(store):
      raise ValueError('idx is longer than the store')
    t = store.tensors
    ptrs = store._ptrs()
    self._call(self._lib.crafter_load_envs, C.byref(ptrs), len(store), store.max_objects, _ptr(t['obs']), _ptr(t['reward']), _ptr(t['done']),
               _ptr(r), _ptr(d), int(d.numel()), _ptr(self.obs), _ptr(self.reward), _ptr(self.done))
    self._keep = (store, r, d)
    if self._unbounded:   # a loaded episode may be longer than any this batch ran: the next _grow_daylight reads the counters
      self._step_bound = self.cfg.n_daylight

  # ------------------------------------------------------------------ measurement
  def enable_phase_stamps(self, enable=True):
    """Debug aid: the step kernel writes shader-clock stamps of its phases into a [N, 8] buffer."""
    self._prof = torch.zeros((self.num_envs, 16), dtype=torch.int64, device=self.device) if enable else None
    self._st.prof = self._prof.data_ptr() if enable else None
    self._native.bind(self._st)
    return self._prof

  def dispatch_order(self):
    """Diagnostics: the order in which the next step() dispatches the envs (numpy int32 [N]; slow envs -- night frame or
    balance step next -- first), or None when this batch keeps none."""
    out = np.empty(self.num_envs, np.int32)
    rc = self._lib.crafter_debug_dispatch_order(self._handle, out.ctypes.data_as(C.c_void_p))
    if rc == 2:
      return None
    self._check(rc)
    return out

  def set_timing(self, enable):
    """Attach HIP start / stop events to the kernels of every following step() (their own execution time)."""
    self._check(self._lib.crafter_set_timing(self._handle, int(bool(enable))))
    self._timing_on = bool(enable)

  def get_timing(self):
    """(sum step-kernel ms, sum reset-kernel ms, launches) since the last call; synchronises."""
    a, b, n = C.c_double(), C.c_double(), C.c_int32()
    self._check(self._lib.crafter_get_timing(self._handle, C.byref(a), C.byref(b), C.byref(n)))
    return a.value, b.value, n.value

  # ------------------------------------------------------------------ host read-back (sync)
  def records(self):
    """Structured numpy copy of every env's scalar record (synchronises)."""
    return state.rec_view(self.state['rec'].cpu().numpy())

  def pool_status(self, stats=True):
    """World pool diagnostics: {'state': 'off' | 'running' | 'failed', 'launched', 'trusted', 'error'} and, with
    stats=True (a small device -> host copy: synchronises), 'adopted' / 'regenerated_inline'."""
    a, b = C.c_uint32(), C.c_uint32()
    rc = self._lib.crafter_pool_status(self._handle, C.byref(a), C.byref(b))
    err = self._lib.crafter_pool_error(self._handle)
    out = {'state': {0: 'off', 1: 'running', 2: 'failed'}.get(rc, 'unknown'), 'launched': a.value,
           'trusted': b.value, 'error': err.decode() if err else ''}
    if stats and 'pool_stats' in self.state:   # synchronises (small device -> host copy)
      s = self.state['pool_stats'].cpu().tolist()
      out['adopted'], out['regenerated_inline'] = int(s[0]), int(s[1])
    return out

  def check_errors(self):
    """Raises if any env hit a sticky device-side error (object-table overflow, bad action...).  (With length=None the
    daylight table grows ahead of the longest episode, _grow_daylight; 'step beyond the daylight table' can only come
    from a caller of the C boundary who never extends it.)  A world pool that was switched off by a HIP error only warns: stepping
    stays correct (finished envs regenerate inline), it is slower.

    Also where the slot table GROWS (the reference's object list has no bound, engine.py:50-58; here `max_objects` slots):
    when an env's table is three quarters full the capacity doubles -- new buffers, a new native handle over them
    (_grow_objects) -- long before an object could be refused, provided the caller comes by here at least every few
    steps (`crafter_amd.Env` does after every step).  A caller who never does keeps the sticky ST_OBJ_OVERFLOW."""
    ps = self.pool_status(stats=False)   # host-side state only: no extra device -> host copy per call
    if ps['state'] == 'failed' and not self._pool_warned:
      import warnings
      warnings.warn(ps['error'], RuntimeWarning)
      self._pool_warned = True
    status = self._rec_i32[:, self._off['status']]
    if self.grow_objects and 4 * int(self._rec_i32[:, self._off['nobj']].max()) > 3 * self.cfg.max_objects:
      self._grow_objects(2 * self.cfg.max_objects)
      status = self._rec_i32[:, self._off['status']]
    bad = torch.nonzero(status).flatten()
    if bad.numel():
      i = int(bad[0])
      bits = int(status[i]) & 0xFFFFFFFF
      names = [v for k, v in abi.ALL_STATUS_NAMES.items() if bits & k]
      raise CrafterDeviceError(f'env {i}: {", ".join(names) or hex(bits)} ({bad.numel()} envs affected)')

  def snapshot(self, i):
    """Canonical host-side dump of env i, comparable with the oracle's snapshot() (tests)."""
    cfg = self.cfg
    r = state.rec_view(self.state['rec'][i:i + 1].cpu().numpy())[0]
    objs = state.objs_view(self.state['objs'][i:i + 1].cpu().numpy())[0]
    R = self.tables.rules
    mat = self.state['mat'][i].cpu().numpy().reshape(cfg.W, cfg.H)
    if self.slot_map_derived:
      occupied = state.occupied_cells(objs, r['nobj'], cfg)
    else:
      occupied = self.state['objmap'][i].cpu().numpy().view(np.uint16).reshape(cfg.W, cfg.H) > 0
    order = self.state['chunk_order'][i].cpu().numpy().view(np.uint16)
    return {
        'step': int(r['step']), 'episode': int(r['episode']), 'mat': mat, 'occupied': occupied,
        'objects': state.live_objects(objs, r['nobj'], r['inv'][R.item_health]),
        'inventory': [int(v) for v in r['inv'][:R.n_items]],
        'achievements': [int(v) for v in r['ach'][:R.n_achievements]],
        'sleeping': bool(r['sleeping']),
        'hunger2': int(r['hunger2']), 'thirst2': int(r['thirst2']), 'fatigue2': int(r['fatigue2']),
        'recover2': int(r['recover2']), 'player_last_health': int(r['player_last_health']),
        'chunk_order': state.chunk_keys(order, r['nchunks_seen'], cfg),
        'mt_key': self.state['mt'][i].cpu().numpy().view(np.uint32), 'mt_pos': int(r['mt_pos']),
    }
