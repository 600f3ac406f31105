"""The gradient-step loop of the reference's offline entry script (train_offline.py:61-123) as a function, for callers
that bring their own environment / logger: load a directory of `.npz` episodes into the HBM replay, then drive
agent.update(replay_iter, step) — through the captured hipGraph when the agent and sampler allow it.

The reference script cannot run as shipped (it calls make_replay_loader with the offline argument shape);
exorl_amd.replay_buffer.make_replay_loader accepts both shapes, so the loop below is the script's loop, not a patch of it.
Environment construction, evaluation roll-outs, video and the CSV/TensorBoard logger stay the caller's (eval_fn / log_fn).
"""
import time

from .replay_buffer import make_replay_loader


def train_offline(agent, replay_dir, num_grad_steps, batch_size, discount, replay_buffer_size=10**7, eval_every_steps=10000,
                  log_every_steps=1000, eval_fn=None, log_fn=None, env=None, sampler='philox', use_graph=True, start_step=0,
                  metric_window=False, mix=None, weighting=None, normalize_obs=False, holdout_every=None, val_batches=0, goal=None):
    """train_offline.py:90-123. Returns the list of (step, metrics) rows that were logged.

    eval_fn(step, agent): called every eval_every_steps (train_offline.py:108-112).
    log_fn(step, metrics): called with the agent's metrics (only non-empty when the agent was built with use_tb=True)
    plus fps / total_time every log_every_steps (train_offline.py:114-121).
    metric_window=True: the metrics are collected on the device (agent.enable_metric_window(), whatever use_tb says) and every logged row
    carries agent.pop_metrics(): the means over the steps since the previous row, which is what the reference's averaging meters write.
    An agent without the window (enable_metric_window() returns False) logs its per-step metrics as before.
    replay_dir may be a list of directories with mix=[fraction per directory]; weighting='episodes'|'transitions' selects the weighted
    sampler (make_offline_replay_loader; both need sampler='philox'). The graph is captured after the weights are in place.
    normalize_obs=True: the TD3+BC authors' state normalisation. The loader z-scores every sampled observation with the dataset's own mean
    and standard deviation in the HBM gather (DeviceReplayLoader) and the agent gets the same pair (agent.set_obs_normalizer) before the
    capture, so eval_fn's agent.act() normalises the environment's observations the way update() saw the data.
    holdout_every=k with val_batches=n > 0: every k-th episode file of each directory is held out of training (DeviceReplayLoader) and, at
    every eval_every_steps boundary, before eval_fn, agent.evaluate(replay_iter.holdout, n) runs n forward-only batches on the held-out
    episodes: its val_* dict goes to the returned rows and to log_fn as (step, dict(val, step=step)). It needs no environment. With
    either left at its default nothing is split, nothing is evaluated and the rows are what they were.
    goal=GoalRelabel(...): goal-conditioned training. The loader relabels every batch in its gather launch ([obs | g] rows, a reached /
    not-reached reward unless reward='keep'; DeviceReplayLoader), so `agent` is built with obs_shape=(O + G,); with normalize_obs it gets
    the widened pair. eval_fn acts on goal.goal_obs(obs, goal_observation)."""
    extra = {k: v for k, v in (('mix', mix), ('weighting', weighting)) if v is not None}
    if normalize_obs:
        extra['normalize_obs'] = True
    validate = holdout_every is not None and int(val_batches) > 0
    if holdout_every is not None:
        extra['holdout_every'] = holdout_every
    if goal is not None:
        extra['goal'] = goal
    loader = make_replay_loader(env, replay_dir, replay_buffer_size, batch_size, 0, discount, sampler=sampler, **extra)
    replay_iter = iter(loader)
    if normalize_obs:
        agent.set_obs_normalizer(*replay_iter.obs_normalizer)
    if hasattr(agent, 'bind_dataset'):          # PRDCAgent: the key table, built through the normaliser, before the capture
        agent.bind_dataset(replay_iter)
    windowed = bool(metric_window) and hasattr(agent, 'enable_metric_window') and agent.enable_metric_window()      # before the capture
    if use_graph and hasattr(agent, 'enable_graph'):
        agent.enable_graph(replay_iter, start_step)      # False (and eager launches) when the pairing cannot be captured
    import torch
    rows = []
    t_start = t_last = time.time()
    for global_step in range(start_step, start_step + num_grad_steps):
        if validate and eval_every_steps and global_step % eval_every_steps == 0:
            val = dict(agent.evaluate(replay_iter.holdout, int(val_batches)), step=global_step)
            rows.append((global_step, val))
            if log_fn is not None:
                log_fn(global_step, val)
        if eval_fn is not None and eval_every_steps and global_step % eval_every_steps == 0:
            eval_fn(global_step, agent)
        metrics = agent.update(replay_iter, global_step)
        if log_every_steps and global_step % log_every_steps == 0:
            torch.cuda.synchronize()
            now = time.time()
            if windowed:
                metrics = agent.pop_metrics()
            row = dict(metrics, fps=log_every_steps / max(now - t_last, 1e-9), total_time=now - t_start, step=global_step)
            t_last = now
            rows.append((global_step, row))
            if log_fn is not None:
                log_fn(global_step, row)
    return rows
