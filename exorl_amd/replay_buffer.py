"""Host-side mirror of the reference's replay interface, backed by the HBM arena in libexorl_hip.so.

Same names, arguments and on-disk format as /root/reference/utils/replay_buffer.py:
  ReplayBufferStorage(data_specs, meta_specs, replay_dir)      :103-150   (episode_{idx}_{len}.npz writer)
  make_replay_loader(storage, max_size, batch_size, num_workers, save_snapshot, nstep, discount)  :260-277
  iter(loader) / next(it) -> (obs, action, reward, discount, next_obs, *meta) batched           :214-239

What is host logic here (file discovery, lexicographic ordering, eviction bookkeeping — :172-212) stays in
Python; what was per-sample Python (episode pick, start index, gathers, n-step loop — :214-235, 30 us/sample)
is one HIP launch per batch. Tensors come back on the GPU (the reference's next step was an H2D copy,
utils.py:55-56, so agents accept either).
"""
import bisect
import os
from collections import OrderedDict, defaultdict
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .engine import ReplayEngine


def episode_len(episode):
    """Transitions in an episode dict: every array carries one extra leading row, the reset step (replay_buffer.py:13-15)."""
    first = next(iter(episode.values()))
    return len(first) - 1


def save_episode(episode, fn):
    """One episode -> one compressed .npz (the reference's on-disk format, replay_buffer.py:18-23). Written under a temporary name and
    renamed, so a loader scanning the directory never sees a half-written file under a name its glob('*.npz') matches."""
    fn = Path(fn)
    tmp = fn.with_name(fn.name + '.part')
    with tmp.open('wb') as f:
        np.savez_compressed(f, **episode)
    os.replace(tmp, fn)


def load_episode(fn):
    """{key: array} of one episode file (replay_buffer.py:25-29); arrays are materialised before the file is closed."""
    with np.load(Path(fn)) as z:
        return {k: z[k] for k in z.files}


def parse_episode_fn(fn):
    """(idx, length) of an episode_{idx}_{len}.npz path: everything the selection rules need is in the name."""
    idx, n = Path(fn).stem.split('_')[1:3]
    return int(idx), int(n)


def _load_or_none(fn):
    try:
        return load_episode(fn)
    except Exception:            # a file still being written: the reference stops the fetch there too (replay_buffer.py:209-212)
        return None


def _load_many(fns, threads):
    """Decodes episode files in order with a bounded look-ahead (a 5-10 M-transition dataset is thousands of
    zlib-compressed .npz files; one decoding thread is what made loading minutes)."""
    if threads <= 1 or len(fns) < 2:
        for fn in fns:
            yield _load_or_none(fn)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=threads) as pool:
        window = 4 * threads
        pending = [pool.submit(_load_or_none, fn) for fn in fns[:window]]
        nxt = len(pending)
        for i in range(len(fns)):
            ep = pending[i].result()
            pending[i] = None
            if nxt < len(fns):
                pending.append(pool.submit(_load_or_none, fns[nxt]))
                nxt += 1
            yield ep


def stack_frames(frames, k):
    """The frame-stack wrapper's deque(maxlen=k) (utils/env_constructor.py:144-188) over one episode: (rows, c0, ...) single frames ->
    (rows, k * c0, ...) observations. Row t is frames max(t - k + 1, 0) .. t along the channel axis, oldest first: the deque is filled
    with the reset frame k times, then takes one frame per step."""
    frames = np.asarray(frames)
    t = np.arange(len(frames))
    return np.concatenate([frames[np.maximum(t - (k - 1 - j), 0)] for j in range(k)], axis=1)


def unstack_frames(obs, k):
    """Inverse of stack_frames: the newest frame obs[:, -c0:] of every row, after checking that `obs` IS a sliding window over one frame
    sequence (row 0 is k copies of one frame; every later row is its predecessor shifted by one frame). Anything else (episodes cut or
    spliced after collection, a wrapper that does not fill with the reset frame) cannot be stored one frame per row without changing
    what is sampled: ValueError naming the first offending row."""
    obs = np.asarray(obs)
    if obs.ndim < 2 or obs.shape[1] % k:
        raise ValueError(f'unstack_frames: {k} frames do not divide the channel axis of observations of shape {obs.shape[1:]}')
    c0 = obs.shape[1] // k
    if k == 1 or len(obs) == 0:
        return obs
    if not np.array_equal(obs[0, :-c0], obs[0, c0:]):
        raise ValueError(f'unstack_frames: row 0 is not {k} copies of the reset frame: the episode is not a frame-stack window')
    bad = np.flatnonzero((obs[1:, :-c0] != obs[:-1, c0:]).reshape(len(obs) - 1, -1).any(axis=1))
    if len(bad):
        raise ValueError(f'unstack_frames: row {int(bad[0]) + 1} does not continue row {int(bad[0])} (its {k - 1} older frames differ): the '
                         'episode is not a frame-stack window')
    return obs[:, -c0:]


class ReplayBufferStorage:
    """Accumulates time-steps and writes finished episodes as episode_{idx}_{len}.npz."""

    def __init__(self, data_specs, meta_specs, replay_dir):
        self._data_specs = data_specs
        self._meta_specs = meta_specs
        self._replay_dir = Path(replay_dir)
        self._replay_dir.mkdir(exist_ok=True)
        self._current_episode = defaultdict(list)
        self._num_episodes = 0
        self._num_transitions = 0
        # episodes finished in this process, kept until an in-process loader has taken them: the HBM sampler ingests them from here
        # instead of re-reading and inflating the file it was just written to; bounded, oldest dropped first
        self._fresh = OrderedDict()
        self._fresh_max = 64
        for fn in self._replay_dir.glob('*.npz'):           # resume counters from what is on disk
            self._num_episodes += 1
            self._num_transitions += parse_episode_fn(fn)[1]

    def __len__(self):
        return self._num_transitions

    def add(self, time_step, meta):
        """One environment step (replay_buffer.py:120-141): meta values and the spec'd fields of `time_step` are appended to the open
        episode; scalars are broadcast to their spec's shape; the step that ends the episode flushes it to disk."""
        cur = self._current_episode
        for key, value in meta.items():
            cur[key].append(value)
        for spec in self._data_specs:
            value = time_step[spec.name]
            if np.isscalar(value):
                value = np.full(spec.shape, value, spec.dtype)
            if value.shape != spec.shape or value.dtype != spec.dtype:
                raise AssertionError(f'{spec.name}: got {value.shape} {value.dtype}, spec says {spec.shape} {spec.dtype}')
            cur[spec.name].append(value)
        if not time_step.last():
            return
        self._current_episode = defaultdict(list)
        self._store_episode({spec.name: np.array(cur[spec.name], spec.dtype) for spec in (*self._data_specs, *self._meta_specs)})

    def _store_episode(self, episode):
        idx, length = self._num_episodes, episode_len(episode)
        self._num_episodes += 1
        self._num_transitions += length
        fn = self._replay_dir / f'episode_{idx}_{length}.npz'
        save_episode(episode, fn)
        self._fresh[fn] = episode
        while len(self._fresh) > self._fresh_max:
            self._fresh.popitem(last=False)


class GoalRelabel:
    """Hindsight goal relabelling in the HBM gather (ReplayEngine.set_goal): what goal= of the iterators, loaders and train_offline takes.

    cols: the observation columns that make a goal, g = o[cols] (1 <= G <= O distinct-or-not indices; range(O) is the whole state).
    Per sample a goal state is drawn: with probability p_cur the state the sample's own trajectory reaches at next_obs, with p_traj a
    state d >= 0 steps behind next_obs in the same episode, with p_rand any state of the arena (a weighted arena picks the episode by its
    weights). horizon_discount=h in (0, 1): d is geometric, P(d = k) = (1 - h) h^k, the mass past the episode's end on its last state;
    None: d is uniform over what is left of the episode. The batches become [obs | g] and [next_obs | g] rows of O + G floats.
    reward: 'neg' (0 where next_obs IS the goal state, else -1; the discount is 0 where it is reached), 'sparse' (1 / 0, same discount)
    or 'keep' (the arena's reward and discount: the goal is context only, as goal-conditioned BC uses it). Reached is equality of the
    indices (episode, time), not a distance. Agents are built with obs_shape=(O + G,) and act on goal_obs(obs, goal_observation)."""
    REWARDS = ('neg', 'sparse', 'keep')

    def __init__(self, cols, p_cur=0.2, p_traj=0.5, p_rand=0.3, horizon_discount=0.99, reward='neg'):
        cols = [cols] if isinstance(cols, (int, np.integer)) else list(cols)
        if not cols:
            raise ValueError('GoalRelabel: cols is empty: a goal is at least one observation column')
        if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0 for c in cols):
            raise ValueError(f'GoalRelabel: cols={cols!r}: expected non-negative integer observation column indices')
        ps = (float(p_cur), float(p_traj), float(p_rand))
        if any(not np.isfinite(p) or p < 0 for p in ps) or abs(sum(ps) - 1.0) > 1e-6:
            raise ValueError(f'GoalRelabel: p_cur={p_cur} p_traj={p_traj} p_rand={p_rand} must be non-negative and sum to 1')
        if horizon_discount is not None and not 0.0 < float(horizon_discount) < 1.0:
            raise ValueError(f'GoalRelabel: horizon_discount={horizon_discount}: expected a value in (0, 1), or None for the uniform horizon')
        if reward not in self.REWARDS:
            raise ValueError(f"GoalRelabel: reward={reward!r}: expected 'neg', 'sparse' or 'keep'")
        self.cols = tuple(int(c) for c in cols)
        self.p_cur, self.p_traj, self.p_rand = ps
        self.horizon_discount = None if horizon_discount is None else float(horizon_discount)
        self.reward = reward

    def __repr__(self):
        return (f'GoalRelabel(cols={list(self.cols)}, p_cur={self.p_cur}, p_traj={self.p_traj}, p_rand={self.p_rand}, '
                f'horizon_discount={self.horizon_discount}, reward={self.reward!r})')

    def goal_obs(self, obs, goal_observation):
        """[obs | goal_observation[cols]] along the last axis, for agent.act(): numpy arrays or torch tensors, a vector or a batch."""
        cols = list(self.cols)
        if hasattr(obs, 'data_ptr'):
            return torch.cat([obs, torch.as_tensor(goal_observation).to(obs)[..., cols]], -1)
        return np.concatenate([np.asarray(obs), np.asarray(goal_observation, np.asarray(obs).dtype)[..., cols]], -1)

    def widen_normalizer(self, mean32, inv32):
        """The (mean, inv) pair of [obs | g] rows from the observation's: [mu | mu[cols]], [inv | inv[cols]]."""
        cols = list(self.cols)
        m, w = np.asarray(mean32, np.float32).reshape(-1), np.asarray(inv32, np.float32).reshape(-1)
        return np.concatenate([m, m[cols]]), np.concatenate([w, w[cols]])


def _goal_args(goal, sampler, frame_stack=None, meta_keys=()):
    """The GoalRelabel a loader or iterator applies (None: none), after refusing what the goal path of the gather cannot honour."""
    if goal is None:
        return None
    if not isinstance(goal, GoalRelabel):
        raise ValueError(f'goal={goal!r}: expected a GoalRelabel')
    if sampler != 'philox':
        raise ValueError(f"goal= needs sampler='philox' (the goals are drawn in the gather kernel): sampler={sampler!r} reproduces the "
                         "reference's index stream, which has no goals")
    if frame_stack is not None and int(frame_stack) > 1:
        raise ValueError(f'goal= with frame_stack={frame_stack}: goals are columns of float32 state rows, not pixels')
    if meta_keys:
        raise ValueError(f'goal= on a storage with meta specs {tuple(meta_keys)}: the goal takes the place behind the observation that '
                         '[obs | meta] rows give them')
    return goal


def _check_goal_rows(out, engine, goal):
    """A goal iterator fills [obs | g] rows: the caller's rows must be exactly O + G floats apart."""
    want = engine.obs_bytes + 4 * len(goal.cols)
    if out.obs_stride != want or out.next_obs_stride != want:
        raise ValueError(f'goal iterator: it writes [obs | g] rows of {engine.obs_bytes // 4} + {len(goal.cols)} floats, the destination has '
                         f'obs_stride={out.obs_stride} / next_obs_stride={out.next_obs_stride} bytes (expected {want}): build the agent '
                         f'with obs_shape=({want // 4},)')


EMPTY_BUFFER = 'replay buffer is empty (random.choice on an empty list, replay_buffer.py:169)'


def _make_arena(loader, episode, capacity_rows, max_episodes):
    """The arena a loader's shard keeps its episodes in, shaped after the first episode it will hold."""
    obs = episode['observation']
    meta_dim = sum(int(np.prod(episode[k].shape[1:])) for k in loader.meta_keys)
    return ReplayEngine(obs.shape[1:], obs.dtype, int(np.prod(episode['action'].shape[1:])), meta_dim, capacity_rows, max_episodes,
                        loader.device, frame_stack=loader.frame_stack or 1)


class _Shard:
    """One reference 'worker': its own resident set, limits and index streams (replay_buffer.py:153-212)."""

    def __init__(self, loader, worker_id):
        self.loader = loader
        self.worker_id = worker_id
        self.size = 0
        self.fns = []                  # sorted, like ReplayBuffer._episode_fns
        self.slot = {}                 # fn -> arena slot
        self.length = {}
        self.since_fetch = loader.fetch_every
        self.frozen = False            # loaded once, never re-scanned: an offline shard, or an arena handed out for graph capture
        self.dir_stamp = None
        self.engine = None
        self.seeded = False
        self.weight = {}               # fn -> float episode weight (episode_weight callable or mix); empty: unit weights

    def _reorder(self):
        """The episode table in `fns` order, and with it the sampling weights: slot ids move when episodes are evicted and stored."""
        ld = self.loader
        self.engine.set_order([self.slot[f] for f in self.fns])
        if ld.weighting is None:
            return
        w = None
        if self.weight:
            w = np.zeros(max(self.slot.values()) + 1, np.float64)      # slots no resident episode holds: 0, out of the quantisation's scale
            for f in self.fns:
                w[self.slot[f]] = self.weight[f]
        self.engine.set_weights(ld.weighting, w)

    def _ensure_engine(self, episode, capacity_rows=None, max_episodes=None):
        """The arena, made when the first episode arrives. Sizes: the caller's (an offline shard knows its files), else the loader's
        max_episodes= / capacity_rows=, else room for max_size transitions."""
        if self.engine is not None:
            return
        ld = self.loader
        max_eps = max_episodes or ld.max_episodes or max(4096, ld.max_size // 64)
        cap = capacity_rows or ld.capacity_rows or (ld.max_size + max_eps + len(episode['observation']) + 1024)
        self.engine = _make_arena(ld, episode, cap, max_eps)

    def _store(self, fn, episode=None, reorder=True):
        ld = self.loader
        if episode is None:
            try:
                episode = load_episode(fn)
            except Exception:
                return False
        n = episode_len(episode)
        self._ensure_engine(episode)
        while n + self.size > ld.max_size:
            early = self.fns.pop(0)                       # lexicographically first (replay_buffer.py:178-182)
            self.engine.evict(self.slot.pop(early))
            self.size -= self.length.pop(early)
            self.weight.pop(early, None)
            early.unlink(missing_ok=True)
        self.slot[fn] = self.engine.append_episode(episode, ld.meta_keys)
        self.length[fn] = n
        if ld.episode_weight is not None:
            self.weight[fn] = float(ld.episode_weight(episode))
        bisect.insort(self.fns, fn)                       # == append + sort (replay_buffer.py:185-186), without re-sorting per episode
        self.size += n
        if reorder:
            self._reorder()
        if not ld.save_snapshot:
            fn.unlink(missing_ok=True)
        return True

    def try_fetch(self):
        ld = self.loader
        if self.frozen or self.since_fetch < ld.fetch_every:
            return
        self.since_fetch = 0
        d = ld.storage._replay_dir
        stamp = os.stat(d).st_mtime_ns
        if stamp == self.dir_stamp and self.fns:
            return                                         # nothing was added since the last scan
        fetched, todo = 0, []
        for fn in sorted(d.glob('*.npz'), reverse=True):  # the reference's selection (replay_buffer.py:196-212) ...
            idx, n = parse_episode_fn(fn)
            if idx % ld.num_workers != self.worker_id:
                continue
            if fn in self.slot:
                break
            if fetched + n > ld.max_size:
                break
            fetched += n
            todo.append(fn)
        # ... decoded by a thread pool (zlib releases the GIL), stored in the reference's order; the episode table is uploaded once
        stored = False
        fresh = getattr(ld.storage, '_fresh', None)
        if fresh and ld.num_workers == 1:                 # one consumer: hand the in-memory copies over and let the storage forget them
            have = {fn: fresh.pop(fn) for fn in todo if fn in fresh}
            rest = iter(_load_many([fn for fn in todo if fn not in have], ld.load_threads))
            episodes = (have[fn] if fn in have else next(rest) for fn in todo)
        else:
            episodes = _load_many(todo, ld.load_threads)
        for fn, episode in zip(todo, episodes):
            if episode is None or not self._store(fn, episode, reorder=False):
                break
            stored = True
        if stored:
            self._reorder()
        self.dir_stamp = os.stat(d).st_mtime_ns


def relabel_episode(env, episode):
    """Rewards recomputed from the stored simulator states under `env`'s task (replay_buffer.py:31-42): ExORL datasets are
    collected reward-free and labelled for the task at load time. `env` is a dm_control-style environment (physics.reset_context /
    set_state, task.get_reward, reward_spec); there is no MuJoCo in this repo, the call is host glue around the caller's env."""
    if 'physics' not in episode:
        raise KeyError("relabel_episode: the episode has no 'physics' states to replay (pass env=None / relabel=False to keep "
                       "the stored rewards)")
    spec = env.reward_spec()
    out = np.empty((len(episode['physics']),) + tuple(spec.shape), spec.dtype)
    for i, state in enumerate(episode['physics']):
        with env.physics.reset_context():
            env.physics.set_state(state)
        out[i] = env.task.get_reward(env.physics)
    episode = dict(episode)
    episode['reward'] = out
    return episode


def mix_weights(lengths, mix, weighting='transitions', nstep=1):
    """Per-episode weight of each dataset d so that a fraction mix[d] of the samples comes from it: mix[d] / M_d, where M_d is the
    dataset's total span sum(max(len - nstep + 1, 0)) under weighting='transitions' (every transition of d equally likely) and its number
    of sampleable episodes (len >= nstep) under weighting='episodes' (every episode of d equally likely). `lengths`: one list of episode
    lengths per dataset. The fractions need not sum to 1 (only their ratios matter); a dataset with a positive fraction and nothing to
    sample is an error."""
    if len(mix) != len(lengths):
        raise ValueError(f'mix has {len(mix)} fractions for {len(lengths)} datasets')
    out = []
    for d, (f, lens) in enumerate(zip(mix, lengths)):
        f = float(f)
        if not np.isfinite(f) or f < 0:
            raise ValueError(f'mix[{d}]={f}: fractions must be finite and non-negative')
        spans = [max(int(n) - nstep + 1, 0) for n in lens]
        m = sum(spans) if weighting == 'transitions' else sum(1 for x in spans if x > 0)
        if f > 0 and m == 0:
            raise ValueError(f'mix[{d}]={f}: dataset {d} has no episode of at least nstep={nstep} transitions')
        out.append(f / m if m else 0.0)
    return out


class _OfflineShard(_Shard):
    """One worker of OfflineReplayBuffer (replay_buffer.py:45-100): a single ASCENDING scan when the first sample is asked for,
    episodes taken until the running size exceeds max_size (:62-63 — checked before each file, so the last one overshoots),
    worker modulo (:65-66), rewards relabelled when an env is given, nothing evicted, re-scanned or deleted. The arena is sized
    from the selected files (lengths are in the names), not from max_size."""

    @staticmethod
    def select(replay_dir, max_size, num_workers, worker_id):
        """The files `_load` keeps (replay_buffer.py:58-75) and their total length, from the names alone."""
        todo, size = [], 0
        for fn in sorted(Path(replay_dir).glob('*.npz')):
            if size > max_size:
                break
            idx, n = parse_episode_fn(fn)
            if idx % num_workers != worker_id:
                continue
            todo.append(fn)
            size += n
        return todo, size

    @classmethod
    def select_many(cls, replay_dirs, max_size, num_workers, worker_id):
        """select() on every directory by itself (each with the whole max_size): [(files, total length), ...] in the order given."""
        return [cls.select(d, max_size, num_workers, worker_id) for d in replay_dirs]

    @staticmethod
    def split_holdout(files, every):
        """(training files, held-out files) of one directory's selection: counted from 0 in the order given, positions every - 1,
        2 * every - 1, ... are held out, every other file trains. From the list alone."""
        if int(every) < 2:
            raise ValueError(f'holdout_every={every}: expected an integer >= 2 (every k-th selected file is held out)')
        files = list(files)
        held = files[int(every) - 1::int(every)]
        return [fn for i, fn in enumerate(files) if (i + 1) % int(every)], held

    holdout_engine = None              # the second, small arena (holdout_every): the held-out episodes of this shard
    holdout_fns = ()

    @staticmethod
    def _arena_sizes(fns):
        """(capacity_rows, max_episodes) of an arena that holds exactly `fns`: an episode takes len + 1 rows."""
        return sum(parse_episode_fn(fn)[1] for fn in fns) + len(fns) + 64, len(fns) + 8

    def _episodes(self, fns):
        """(fn, episode) of every file of `fns` in order: decoded by the thread pool, rewards relabelled when the loader asks for it."""
        ld = self.loader
        for fn, episode in zip(fns, _load_many(fns, ld.load_threads)):
            if episode is None:
                raise IOError(f'offline dataset: cannot read {fn}')
            yield fn, (relabel_episode(ld.env, episode) if ld.relabel else episode)

    def _load_holdout(self, held):
        """The held-out files into an arena of their own, sampled transition-uniformly (the training side's weights do not apply)."""
        ld = self.loader
        self.holdout_fns = list(held)
        if not held:
            return
        slots = []
        for fn, episode in self._episodes(held):
            if self.holdout_engine is None:
                self.holdout_engine = _make_arena(ld, episode, *self._arena_sizes(held))
            slots.append(self.holdout_engine.append_episode(episode, ld.meta_keys))
        self.holdout_engine.set_order(slots)
        self.holdout_engine.set_weights('transitions', None)

    def try_fetch(self):
        if self.frozen or self.engine is not None:
            return
        ld = self.loader
        picks = [t for t, _ in self.select_many(ld.storage._replay_dirs, ld.max_size, ld.num_workers, self.worker_id)]
        held = []
        if ld.holdout_every:      # per directory, in select's ascending order; mix and the weights see the training files only
            split = [self.split_holdout(t, ld.holdout_every) for t in picks]
            picks, held = [train for train, _ in split], [fn for _, h in split for fn in h]
        todo = [fn for t in picks for fn in t]
        if not todo:
            return
        self._load_holdout(held)
        if ld.mix is not None:                   # normalised over what THIS shard holds of each dataset
            per = mix_weights([[parse_episode_fn(fn)[1] for fn in t] for t in picks], ld.mix, ld.weighting, ld.nstep)
            self.weight = {fn: w for t, w in zip(picks, per) for fn in t}
        sizes = self._arena_sizes(todo)
        for fn, episode in self._episodes(todo):
            self._ensure_engine(episode, *sizes)
            self.slot[fn] = self.engine.append_episode(episode, ld.meta_keys)
            self.length[fn] = episode_len(episode)
            if ld.episode_weight is not None:
                self.weight[fn] = float(ld.episode_weight(episode))
            self.fns.append(fn)
            self.size += self.length[fn]
        self._reorder()
        self.frozen = True                       # loaded once (replay_buffer.py:78-80)


def _weighting_args(sampler, weighting, episode_weight, mix=None):
    """The weighting mode a loader applies (None: it never touches the arena's weights), after refusing what cannot be honoured."""
    if weighting is None and episode_weight is None and mix is None:
        return None
    if weighting not in (None, 'episodes', 'transitions'):
        raise ValueError(f"weighting={weighting!r}: expected 'episodes' or 'transitions'")
    if sampler != 'philox':
        raise ValueError(f"weighting / episode_weight / mix need sampler='philox': sampler={sampler!r} reproduces the reference's "
                         'unweighted index stream')
    if episode_weight is not None and not callable(episode_weight):
        raise ValueError('episode_weight must be a callable: episode dict -> float')
    if episode_weight is not None and mix is not None:
        raise ValueError('mix sets the episode weights itself: pass either mix or episode_weight')
    return weighting or 'episodes'


class DeviceReplayLoader:
    """What make_replay_loader returns: iterable whose iterator yields device-resident minibatches.

    weighting='episodes'|'transitions' and episode_weight (a callable: episode dict -> non-negative float, e.g.
    `lambda ep: 4.0 if ep['constraint'].any() else 1.0`) select ReplayEngine.set_weights' weighted sampling; they are re-applied
    whenever episodes are stored, evicted or re-ordered, and need sampler='philox'. mix: see make_offline_replay_loader.

    frame_stack=k (the run's cfg.frame_stack; None or 1: rows are stored as they come): the episodes on disk and from the storage are
    the frame-stack wrapper's (k * c0, H, W) observations; the arena keeps one (c0, H, W) frame per step, 1/k of the memory and of the
    upload, and the gather rebuilds the stacks: the batches are byte-identical. An episode that is not such a window raises ValueError
    at ingest (unstack_frames).

    normalize_obs=True (offline loaders, float32 states): after the one-shot load the iterator takes the column moments of EVERY shard
    arena it holds (ReplayEngine.obs_moments: all rows of all resident episodes, several mix directories in one arena included), exchanges
    them between the ranks of an initialised torch.distributed (all_gather_object of a handful of doubles; `gather`, a callable
    own partials -> [partials of rank 0, partials of rank 1, ...], replaces that exchange), merges them with utils.combine_moments, ranks in
    rank order and each rank's shards in shard order (training arenas only: a hold-out split's arenas get the pair, not a vote), and sets utils.obs_normalizer(count, mean, M2, norm_eps) on all its arenas: every
    sampled obs / next_obs is (x - mean) / (std + norm_eps) of the whole dataset, whatever the sampler. The iterator's .obs_normalizer is
    the (mean32, inv32) pair to hand to agent.set_obs_normalizer, so that act() sees what update() trained on. It is in place before
    .engine is handed to agent.enable_graph. A growing online buffer is refused: its statistic would move under the policy.

    holdout_every=k (offline loaders, k >= 2): of the files _OfflineShard.select keeps, per directory and in its ascending order, every
    k-th (positions k - 1, 2k - 1, ... counted from 0) goes to a second, small arena of the same shard and never trains; the rest load
    as before. weighting, episode_weight and mix apply to the training arena only (mix normalises over the training files); the hold-out
    arena is sampled transition-uniformly by the Philox sampler, whatever the loader's. iter(loader).holdout is the iterator over it
    (HoldoutIterator: same next() / sample_into() contract, same nstep and discount, a seed derived from the loader's), None without
    holdout_every. With normalize_obs the moments are the training arenas' alone and the same pair is set on the hold-out arenas."""

    def __init__(self, storage, max_size, batch_size, num_workers, save_snapshot, nstep, discount, fetch_every=1000,
                 device='cuda', sampler='mt19937', seed=None, worker_ids=None, max_episodes=None, capacity_rows=None, static=False,
                 load_threads=None, offline=False, env=None, relabel=False, weighting=None, episode_weight=None, mix=None,
                 frame_stack=None, normalize_obs=False, norm_eps=1e-3, gather=None, holdout_every=None, goal=None):
        self.goal = _goal_args(goal, sampler, frame_stack, tuple(s.name for s in getattr(storage, '_meta_specs', ())))
        if holdout_every is not None:
            if not offline:
                raise ValueError('holdout_every needs an offline loader (make_offline_replay_loader): an online buffer evicts and re-scans, '
                                 'a fixed split of its files does not exist')
            if isinstance(holdout_every, bool) or int(holdout_every) != holdout_every or int(holdout_every) < 2:
                raise ValueError(f'holdout_every={holdout_every!r}: expected an integer >= 2 (every k-th selected file is held out)')
        self.holdout_every = None if holdout_every is None else int(holdout_every)
        if frame_stack is not None and not 1 <= int(frame_stack) <= 16:
            raise ValueError(f'frame_stack={frame_stack}: expected 1 .. 16')
        if normalize_obs and not offline:
            raise ValueError('normalize_obs=True needs an offline loader (make_offline_replay_loader): the statistic of a growing online '
                             'buffer would move under the policy')
        if normalize_obs and frame_stack is not None and int(frame_stack) > 1:
            raise ValueError(f'normalize_obs=True with frame_stack={frame_stack}: only float32 state observations are normalised (the pixel '
                             'encoder does its own /255 - 0.5)')
        self.normalize_obs, self.norm_eps, self.gather = bool(normalize_obs), float(norm_eps), gather
        self.frame_stack = None if frame_stack is None else int(frame_stack)
        self.weighting, self.episode_weight, self.mix = _weighting_args(sampler, weighting, episode_weight, mix), episode_weight, mix
        self.storage = storage
        self.offline, self.env, self.relabel = offline, env, relabel      # OfflineReplayBuffer semantics (see _OfflineShard)
        self.static = static                # the directory will not change (offline datasets): load once, never re-scan
        self.num_workers = max(1, num_workers)
        self.max_size = max_size // self.num_workers          # replay_buffer.py:262
        self.batch_size = batch_size
        self.save_snapshot = save_snapshot
        self.nstep = nstep
        self.discount = discount
        self.fetch_every = fetch_every
        self.device = device
        self.sampler = {'mt19937': L.SAMPLER_MT19937, 'philox': L.SAMPLER_PHILOX}[sampler]
        self.seed = seed
        self.meta_keys = tuple(s.name for s in getattr(storage, '_meta_specs', ()))
        self.max_episodes = max_episodes
        self.capacity_rows = capacity_rows
        self.load_threads = load_threads if load_threads is not None else min(16, os.cpu_count() or 1)      # episode decode pool
        # which reference workers this process plays: all of them (single process) or a subset (one per DP rank)
        self.worker_ids = list(range(self.num_workers)) if worker_ids is None else list(worker_ids)

    def __iter__(self):
        return DeviceReplayIterator(self)

    def goal_obs(self, obs, goal_observation):
        """[obs | goal_observation[cols]] of a goal= loader, for agent.act() (GoalRelabel.goal_obs)."""
        if self.goal is None:
            raise ValueError('goal_obs: the loader was made without goal=')
        return self.goal.goal_obs(obs, goal_observation)


def start_pair_batches(n_episodes, batch):
    """The (position, 1) pairs of episodes 0 .. n_episodes - 1 of one arena's order table, cut into batches of `batch`: yields
    (pairs, valid_rows) with pairs an int32 (batch, 2) array for the GIVEN sampler at nstep = 1 (idx 1 gathers row 0 of the episode as obs) and
    valid_rows the rows that are episodes. The last batch is padded with copies of position 0 (a pair the sampler accepts); a consumer leaves
    rows >= valid_rows out. Pure: no device, no arena."""
    n, batch = int(n_episodes), int(batch)
    if batch < 1:
        raise ValueError(f'start_pair_batches: batch={batch}')
    for first in range(0, n, batch):
        valid = min(batch, n - first)
        pairs = np.zeros((batch, 2), np.int32)
        pairs[:valid, 0] = np.arange(first, first + valid, dtype=np.int32)
        pairs[:, 1] = 1
        yield pairs, valid


def _ensure_returns(engine, discount):
    """The arena's return-to-go column, standing and built with `discount`: built on the first request and again once it is stale (an
    online loader's fetch appends, evicts and reorders) or was built with another discount."""
    _, gamma, _, valid = engine.returns_info()
    if not valid or np.float32(gamma).tobytes() != np.float32(discount).tobytes():
        engine.build_returns(discount)


class _EpisodeStarts:
    """What FQEAgent.value() asks of an HBM iterator: every resident episode of every arena it samples from, once, and their returns.
    Neither touches an arena's Philox stream (the GIVEN sampler draws nothing), so a captured graph bound to the iterator is undisturbed."""

    def _arenas(self):
        raise NotImplementedError

    def episode_starts(self, batch=None, out=None):
        """Yields (pairs, valid_rows) per batch (start_pair_batches), arena after arena in shard order; a batch never straddles two arenas.
        With `out` (an exorl_batch_out, e.g. an agent's batch slots) each batch has been gathered into it before it is yielded: GIVEN
        sampler, nstep = 1, so obs is the episode's first observation, normalised if the arena normalises."""
        batch = batch or self.batch_size
        for eng in self._arenas():
            for pairs, valid in start_pair_batches(eng.num_episodes(), batch):
                if out is not None:
                    eng.sample_into(out, batch, 1, self.discount, L.SAMPLER_GIVEN, pairs)
                yield pairs, valid

    def episode_returns(self):
        """float64 discounted returns of every episode episode_starts() enumerates, in its order (ReplayEngine.episode_returns at the
        iterator's discount): the behaviour policy's value, the anchor an FQE estimate is read against."""
        return np.concatenate([eng.episode_returns(self.discount) for eng in self._arenas()])


class DeviceReplayIterator(_EpisodeStarts):
    goal = None             # the loader's GoalRelabel: what agents read, a goal iterator fills [obs | g] rows

    def __init__(self, loader):
        self.loader = loader
        self.shards = [(_OfflineShard if loader.offline else _Shard)(loader, w) for w in loader.worker_ids]
        self.turn = 0
        # what agent.enable_graph reads; .engine is only set for a static single-shard dataset (see static_engine)
        self.sampler, self.nstep, self.discount, self.batch_size = loader.sampler, loader.nstep, loader.discount, loader.batch_size
        self._normalizer = None
        self._holdout = None
        self.goal = loader.goal

    @property
    def holdout(self):
        """The iterator over the held-out episodes of a holdout_every loader (HoldoutIterator), None otherwise. The first look loads
        every shard; a split that left a shard nothing to sample raises ValueError."""
        ld = self.loader
        if ld.holdout_every is None:
            return None
        if self._holdout is None:
            for shard in self.shards:
                self._load_shard(shard)
            self._ensure_normalizer()
            for shard in self.shards:
                if shard.holdout_engine is None or not any(parse_episode_fn(fn)[1] >= ld.nstep for fn in shard.holdout_fns):
                    raise ValueError(f'holdout_every={ld.holdout_every}: the split left worker {shard.worker_id} no held-out episode of at '
                                     f'least nstep={ld.nstep} transitions ({len(shard.fns)} training files, {len(shard.holdout_fns)} held out): '
                                     'use a smaller holdout_every or more episodes')
            self._holdout = HoldoutIterator(self)
        return self._holdout

    def _seed_base(self):
        """What every index stream of this iterator is derived from: the loader's seed, else word 0 of NumPy's global state."""
        ld = self.loader
        return int(np.random.get_state()[1][0]) if ld.seed is None else int(ld.seed)

    def _seed(self, shard):
        ld = self.loader
        if ld.sampler == L.SAMPLER_MT19937 and ld.num_workers == 1 and ld.seed is None:
            shard.engine.seed_mt_from_globals()              # continue random / np.random exactly (num_workers=0 case)
        else:
            seed = self._seed_base() + shard.worker_id       # _worker_init_fn: seed = np state word 0 + worker_id
            if ld.sampler == L.SAMPLER_MT19937:
                shard.engine.seed_mt_ints(seed, seed & 0xFFFFFFFF)
            else:
                shard.engine.seed_philox(seed)
        shard.seeded = True

    def _load_shard(self, shard):
        """The scan that the shard's first sample would trigger, and its index streams: every way into the iterator comes through here,
        so a shard is loaded and seeded once whichever of next(), sample_into(), .engine, .obs_normalizer and .holdout is touched first."""
        if shard.engine is None:
            shard.try_fetch()
            if shard.engine is None:
                raise IndexError(EMPTY_BUFFER)
        if not shard.seeded:
            self._seed(shard)
        if self.goal is not None and shard.engine.goal is not self.goal:
            shard.engine.set_goal(self.goal)

    def goal_obs(self, obs, goal_observation):
        return self.loader.goal_obs(obs, goal_observation)

    def _arenas(self):
        for shard in self.shards:
            self._load_shard(shard)
        self._ensure_normalizer()
        return [shard.engine for shard in self.shards]

    @property
    def obs_normalizer(self):
        """(mean32, inv32) of a normalize_obs=True loader, for agent.set_obs_normalizer; None otherwise. The first look loads every shard,
        takes and exchanges the moments and sets the normaliser on all the shard arenas (DeviceReplayLoader). On a goal= loader the pair
        is widened to the [obs | g] rows the agent sees."""
        pair = self._ensure_normalizer()
        return pair if pair is None or self.goal is None else self.goal.widen_normalizer(*pair)

    def _ensure_normalizer(self):
        ld = self.loader
        if not ld.normalize_obs or self._normalizer is not None:
            return self._normalizer
        from .utils import combine_moments, obs_normalizer
        for shard in self.shards:
            self._load_shard(shard)
        own = [shard.engine.obs_moments() for shard in self.shards]
        gather = ld.gather
        if gather is None and torch.distributed.is_available() and torch.distributed.is_initialized():
            def gather(parts):
                out = [None] * torch.distributed.get_world_size()
                torch.distributed.all_gather_object(out, parts)
                return out
        ranks = [own] if gather is None else gather(own)
        count, mean, m2 = combine_moments([part for parts in ranks for part in parts])
        self._normalizer = obs_normalizer(count, mean, m2, ld.norm_eps)
        for shard in self.shards:
            shard.engine.set_obs_normalizer(*self._normalizer)
            if shard.holdout_engine is not None:      # validation sees the inputs the policy sees; the held-out rows had no part in the moments
                shard.holdout_engine.set_obs_normalizer(*self._normalizer)
        return self._normalizer

    @property
    def engine(self):
        """The HBM arena, when sampling from it can be captured into the agent's hipGraph: a static directory held by one
        shard with the Philox sampler (no host-side re-scan or MT19937 draws between steps). None otherwise."""
        ld = self.loader
        if not (ld.static and len(self.shards) == 1 and ld.sampler == L.SAMPLER_PHILOX):
            return None
        shard = self.shards[0]
        self._load_shard(shard)
        self._ensure_normalizer()           # normalize_obs: in place before the arena is captured
        shard.frozen = True                 # the captured graph samples without passing through the fetch counter
        return shard.engine

    def __iter__(self):
        return self

    def _segments(self, shard, batch):
        """Splits a batch where the reference would re-scan the directory mid-batch: it checks before EVERY
        sample (replay_buffer.py:216,193) and scans once `fetch_every` samples have been drawn. A frozen shard never re-scans:
        the whole batch is one segment."""
        self._load_shard(shard)
        if shard.frozen:
            yield 0, batch
            return
        done = 0
        while done < batch:
            if shard.since_fetch >= self.loader.fetch_every:
                shard.try_fetch()
            n = min(self.loader.fetch_every - shard.since_fetch, batch - done)
            yield done, n
            shard.since_fetch += n
            done += n

    def sample_into(self, out, batch=None, mc_return=None):
        """Zero-copy path: writes the next minibatch straight into caller-owned device memory (exorl_batch_out). mc_return: a (batch,)
        float32 device tensor that takes each sample's Monte-Carlo return-to-go at the loader's discount, written by the same gather launch;
        the shard's column is built on the first request and again when a fetch made it stale. An episode cut by a time limit gets the
        return of its recorded remainder, a lower bound only where rewards are >= 0."""
        ld = self.loader
        batch = batch or ld.batch_size
        self._ensure_normalizer()           # normalize_obs: set on every shard before the first sample
        shard = self.shards[self.turn % len(self.shards)]
        self.turn += 1
        for start, n in self._segments(shard, batch):
            if not shard.fns:                                 # loaded, then emptied by an eviction
                raise IndexError(EMPTY_BUFFER)
            if self.goal is not None:
                _check_goal_rows(out, shard.engine, self.goal)
            seg = L.BatchOut(out.obs + start * out.obs_stride, out.obs_stride,
                             out.action + start * out.action_stride * 4, out.action_stride,
                             out.reward + start * 4, out.discount + start * 4,
                             out.next_obs + start * out.next_obs_stride, out.next_obs_stride,
                             (out.meta + start * out.meta_stride * 4) if out.meta else None, out.meta_stride,
                             (out.next_action + start * out.next_action_stride * 4) if out.next_action else None, out.next_action_stride,
                             (out.next_valid + start * 4) if out.next_valid else None)
            kw = {} if self.goal is None else {'goal': True}
            if mc_return is None:
                shard.engine.sample_into(seg, n, ld.nstep, ld.discount, ld.sampler, **kw)
            else:
                _ensure_returns(shard.engine, ld.discount)
                shard.engine.sample_into(seg, n, ld.nstep, ld.discount, ld.sampler, mc_return=mc_return[start:start + n], **kw)

    def __next__(self):
        ld = self.loader
        B = ld.batch_size
        self._ensure_normalizer()
        shard = self.shards[self.turn % len(self.shards)]
        self._load_shard(shard)                               # first batch: the scan that sample 0 would trigger
        res, out = shard.engine.alloc_batch(B) if self.goal is None else shard.engine.alloc_batch(B, len(self.goal.cols))
        self.sample_into(out, B)
        if len(res) == 5:
            return res
        meta, res, o = res[5], list(res[:5]), 0               # one tensor per meta spec, like the reference's *meta
        for spec in ld.storage._meta_specs:
            w = int(np.prod(spec.shape))
            res.append(meta[:, o:o + w].reshape((B,) + tuple(spec.shape)))
            o += w
        return tuple(res)


class ArenaIterator(_EpisodeStarts):
    """Iterator over an already-filled ReplayEngine (no directory behind it): what bench.py and callers that
    ingest datasets themselves use. Same next()/sample_into() contract as DeviceReplayIterator."""
    goal = None

    def __init__(self, engine, batch_size, nstep, discount, sampler='philox', weighting=None, episode_weight=None, episodes=None, goal=None):
        """weighting / episode_weight: as DeviceReplayLoader's, applied once here through engine.set_weights. The arena keeps no episode
        dicts, so a callable episode_weight needs `episodes`: the dicts that were appended, indexed by slot id.
        goal: a GoalRelabel, set on the arena here (engine.set_goal): the iterator then fills and yields [obs | g] rows (DeviceReplayLoader)."""
        self.engine, self.batch_size, self.nstep, self.discount = engine, batch_size, nstep, discount
        self.goal = _goal_args(goal, sampler)
        if self.goal is not None:
            engine.set_goal(self.goal)
        self.sampler = {'mt19937': L.SAMPLER_MT19937, 'philox': L.SAMPLER_PHILOX}[sampler]
        mode = _weighting_args(sampler, weighting, episode_weight)
        if mode is not None:
            if episode_weight is not None and episodes is None:
                raise ValueError('ArenaIterator: episode_weight needs episodes=[episode dict per slot id]')
            engine.set_weights(mode, None if episode_weight is None else [float(episode_weight(ep)) for ep in episodes])

    def __iter__(self):
        return self

    def _next_engine(self):
        return self.engine

    def _arenas(self):
        return [self.engine]

    def sample_into(self, out, batch=None, mc_return=None):
        """mc_return: a (batch,) float32 device tensor that takes each sample's Monte-Carlo return-to-go at this iterator's discount, written
        by the same gather launch; the arena's column is built on the first request and again when it is stale. An episode cut by a time limit
        gets the return of its recorded remainder, a lower bound only where rewards are >= 0."""
        eng = self._next_engine()
        if self.goal is not None:
            _check_goal_rows(out, eng, self.goal)
        if mc_return is not None:
            _ensure_returns(eng, self.discount)
        eng.sample_into(out, batch or self.batch_size, self.nstep, self.discount, self.sampler, mc_return=mc_return,
                        **({} if self.goal is None else {'goal': True}))

    def __next__(self):
        if self.goal is None:
            return self._next_engine().sample(self.batch_size, self.nstep, self.discount, self.sampler)
        eng = self._next_engine()
        res, out = eng.alloc_batch(self.batch_size, len(self.goal.cols))
        eng.sample_into(out, self.batch_size, self.nstep, self.discount, self.sampler, goal=True)
        return res

    def goal_obs(self, obs, goal_observation):
        """[obs | goal_observation[cols]] of a goal iterator, for agent.act() (GoalRelabel.goal_obs)."""
        if self.goal is None:
            raise ValueError('goal_obs: the iterator was made without goal=')
        return self.goal.goal_obs(obs, goal_observation)


HOLDOUT_SEED_SALT = 0x5851F42D4C957F2D       # the hold-out arenas' Philox seed: the training arena's xor this, so the two streams differ


class HoldoutIterator(ArenaIterator):
    """ArenaIterator over the hold-out arenas of a holdout_every loader, shard after shard in turn: the loader's nstep and discount, the
    Philox sampler with transition-uniform weights (set at load)."""

    def __init__(self, parent):
        ld = parent.loader
        self.batch_size, self.nstep, self.discount, self.sampler = ld.batch_size, ld.nstep, ld.discount, L.SAMPLER_PHILOX
        self.engines = [shard.holdout_engine for shard in parent.shards]
        self.goal = ld.goal                       # validation batches are relabelled by the training rule
        for shard in parent.shards:
            if self.goal is not None:
                shard.holdout_engine.set_goal(self.goal)
            shard.holdout_engine.seed_philox(((parent._seed_base() + shard.worker_id) ^ HOLDOUT_SEED_SALT) & 0x7FFFFFFFFFFFFFFF)
        self.turn = 0

    def _next_engine(self):
        eng = self.engines[self.turn % len(self.engines)]
        self.turn += 1
        return eng

    def _arenas(self):
        return list(self.engines)


def make_replay_loader(storage, max_size, batch_size, num_workers, save_snapshot, nstep=None, discount=None, **kw):
    """replay_buffer.py:260-261 signature. Also accepts the 6-argument offline call shape that
    train_offline.py:90-93 uses — (env, replay_dir, max_size, batch_size, num_workers, discount) — which the
    reference's own 7-parameter function rejects; there replay_dir may be a list of directories with mix=[...]
    (make_offline_replay_loader)."""
    if discount is None and isinstance(max_size, (str, os.PathLike, list, tuple)):
        env, replay_dir, max_size, batch_size, num_workers, discount = (storage, max_size, batch_size, num_workers,
                                                                       save_snapshot, nstep)
        return make_offline_replay_loader(env, replay_dir, max_size, batch_size, num_workers, discount, **kw)
    return DeviceReplayLoader(storage, max_size, batch_size, num_workers, save_snapshot, nstep, discount, **kw)


class _DirStorage:
    """Minimal storage stand-in for a directory of pre-collected episodes (offline datasets)."""

    def __init__(self, replay_dir, meta_specs=()):
        many = isinstance(replay_dir, (list, tuple))
        self._replay_dirs = [Path(d) for d in replay_dir] if many else [Path(replay_dir)]
        self._replay_dir = self._replay_dirs[0]
        self._meta_specs = tuple(meta_specs)


def make_offline_replay_loader(env, replay_dir, max_size, batch_size, num_workers, discount, relabel=None, mix=None, **kw):
    """replay_buffer.py:246-258 with OfflineReplayBuffer's semantics (:45-100): ascending one-shot load up to the first episode
    that takes the size past max_size // workers, nstep = 1, files never touched. relabel=None follows the reference's intent —
    rewards are relabelled through `env` (relabel_episode, :31-42) whenever an env is given; pass relabel=False (or env=None) to
    train on the stored rewards. The reference's own class fails before loading anything (`_relable_reward` typo, :72 vs :84).

    replay_dir may be a list of directories (datasets collected by different agents, or the reward / constraint episode sets that
    prioritized_sampling.py copies into one directory): each is selected by itself with the rule above and the same max_size, ascending
    within a directory, directories in the order given, all in one arena. mix=[f_0, f_1, ...] (needs sampler='philox') gives the
    fraction of samples drawn from each: every episode of dataset d gets the weight f_d / M_d (mix_weights), where
      weighting='transitions': M_d = the dataset's total span, sum of (len - nstep + 1) over its episodes: all its transitions equally likely;
      weighting='episodes' (the default): M_d = its number of sampleable episodes: all its episodes equally likely, then a uniform start.
    Under data parallelism (worker_ids) every rank normalises over its own shard of each dataset. Without mix the datasets are simply
    concatenated under `weighting`. A directory may be listed only once. weighting= and episode_weight= are DeviceReplayLoader's, and so
    is holdout_every=k: every k-th selected file of each directory is held out for agent.evaluate(iter(loader).holdout) and mix is
    normalised over the files that train."""
    many = isinstance(replay_dir, (list, tuple))
    if mix is not None and (not many or len(mix) != len(replay_dir)):
        raise ValueError('make_offline_replay_loader: mix needs a list of directories and one fraction per directory')
    if many and not replay_dir:
        raise ValueError('make_offline_replay_loader: empty list of directories')
    if many and len({Path(d).resolve() for d in replay_dir}) != len(replay_dir):
        raise ValueError('make_offline_replay_loader: a directory is listed twice (episodes are keyed by their path): list it once and '
                         'give it a larger mix fraction or episode_weight instead')
    if relabel is None:
        relabel = env is not None
    if relabel and env is None:
        raise ValueError('make_offline_replay_loader: relabel=True needs the env whose task defines the reward')
    return DeviceReplayLoader(_DirStorage(replay_dir), max_size, batch_size, num_workers, True, 1, discount, static=True, offline=True,
                              env=env, relabel=bool(relabel), mix=None if mix is None else [float(f) for f in mix], **kw)
