"""Digests of everything the agent classes compute, for comparing two trees bit for bit (a refactor of exorl_amd/agents.py or engine.py
must leave every line equal). Run it from each tree in a fresh process per listing, then compare the listings:

    python tools/agent_digests.py part1 OUT.txt [PICKLE_DIR]   every agent class, three update() calls; writes pickle.dumps(agent) per case
    python tools/agent_digests.py part2 OUT.txt PICKLE_DIR     loads those pickles (written by either tree), one more update()
    python tools/agent_digests.py part3 OUT.txt                the five two-process gloo workers of tests/, every array and json they save
    python tools/agent_digests.py grid OUT.txt                 one update() of every case of the state agents' kernel dispatch grids, per route
    python tools/agent_digests.py modes OUT.txt                one state-agent handle through every driver of its step in turn (see modes)
    python tools/agent_digests.py summary PARENT.txt THIS.txt  the per-case table profiles/*_digests.txt keep of two listings (see summary)
    python tools/agent_digests.py pixel_modes OUT.txt          one pixel handle through every driver of its step in turn (see pixel_modes)
    python tools/agent_digests.py replay OUT.txt               the replay loaders, online and offline: batches and index pairs (see replay)
    python tools/agent_digests.py compare A.txt B.txt          "N entries, K differ" and every differing line; exit status 1 if K > 0

A listing has one line per entry, `case what value`; a value is the first 32 hex digits of a sha256 or a float.hex(). Inputs come from
tests/_synth.py and seeded numpy streams only. The state engines' derived weight images (AgentEngine.weight_images) are listed one by one next
to the whole-workspace digest; against a listing of a tree from before that export they show as `<missing>`. Needs a GPU (there is no CPU path)."""
import hashlib
import json
import os
import pickle
import socket
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

O, A, H, B = 24, 6, 256, 256                        # states
PC, PHW, PF, PH, PB = 3, 64, 32, 128, 64            # pixels: the two-process workers' frames and widths
OFFLINE = ['td3_bc', 'td3', 'bc', 'crr', 'cql', 'cql_lagrange']
OFFLINE_LATER = ['iql', 'fqe', 'prdc']              # their cases follow every older one, so that a listing's older part keeps its order
MODULES = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
META = {'states': {'diayn': 16, 'aps': 10, 'smm': 4}, 'pixels': {'diayn': 8, 'aps': 5, 'smm': 4}}
PRECISIONS = {'states': ('fp32', 'bf16', 'bf16x3', 'bf16x6'), 'pixels': ('fp32', 'bf16x6')}


def sha(x):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x).tobytes()
    if isinstance(x, str):
        x = x.encode()
    return hashlib.sha256(x).hexdigest()[:32]


def build(kind, obs_type, reward_free, precision, use_tb=True):
    import torch
    from exorl_amd import agents
    torch.manual_seed(7)
    if kind in OFFLINE + OFFLINE_LATER:
        a = ('x', (O,), (A,), 'cuda:0', 1e-4, H, 0.01)
        if kind == 'iql':
            return agents.IQLAgent(*a, '0.2', 1, B, use_tb, precision=precision)
        if kind == 'fqe':           # the policy it scores: a TD3+BC agent from the same seed
            return agents.FQEAgent(*a, 1, B, use_tb, precision=precision).set_policy(build('td3_bc', obs_type, reward_free, precision, use_tb))
        if kind == 'prdc':          # searches a bound table: bind_prdc() before the first update()
            return agents.PRDCAgent(*a, '0.2', 1, B, 0.3, use_tb, 2.5, beta=2.0, precision=precision)
        if kind == 'td3_bc':
            return agents.TD3BCAgent(*a, '0.2', 1, B, 0.3, use_tb, 2.5, precision=precision)
        if kind == 'td3':
            return agents.TD3Agent(*a, '0.2', 1, B, 0.3, use_tb, precision=precision)
        if kind == 'crr':
            return agents.CRRAgent(*a, 4, 'exp', '0.2', 1, B, 0.3, use_tb, precision=precision)
        if kind == 'bc':
            return agents.BCAgent('x', (O,), (A,), 'cuda:0', 1e-4, H, B, '0.2', use_tb, precision=precision)
        return agents.CQLAgent(*a, 1, B, use_tb, 0.01, 3, 5.0, kind == 'cql_lagrange', precision=precision)
    pix = obs_type == 'pixels'
    kw = dict(name=kind, reward_free=reward_free, obs_type=obs_type, obs_shape=(PC, PHW, PHW) if pix else (O,), action_shape=(A,),
              device='cuda:0', lr=1e-4, feature_dim=PF if pix else 50, hidden_dim=PH if pix else H, critic_target_tau=0.01, num_expl_steps=0,
              update_every_steps=1, stddev_schedule=0.2, nstep=3, batch_size=PB if pix else B, stddev_clip=0.3, init_critic=True, use_tb=use_tb,
              use_wandb=False, precision=precision)
    M = META[obs_type].get(kind, 0)
    knn = dict(knn_rms=True, knn_k=12, knn_avg=True, knn_clip=0.0)
    if kind == 'ddpg':
        return agents.DDPGAgent(**kw)
    if kind == 'rnd':
        return agents.RNDAgent(rnd_rep_dim=32, update_encoder=True, rnd_scale=1.0, **kw)
    if kind == 'icm':
        return agents.ICMAgent(icm_scale=1.0, update_encoder=True, **kw)
    if kind == 'icm_apt':
        return agents.ICMAPTAgent(icm_scale=1.0, update_encoder=True, icm_rep_dim=32, **knn, **kw)
    if kind == 'disagreement':
        return agents.DisagreementAgent(update_encoder=True, **kw)
    if kind == 'diayn':
        return agents.DIAYNAgent(update_skill_every_step=50, skill_dim=M, diayn_scale=1.0, update_encoder=True, skill_type='uniform', **kw)
    if kind == 'aps':
        return agents.APSAgent(update_task_every_step=50, sf_dim=M, num_init_steps=0, lstsq_batch_size=64, update_encoder=True, **knn, **kw)
    if kind == 'smm':
        return agents.SMMAgent(z_dim=M, sp_lr=1e-3, vae_lr=1e-2, vae_beta=0.5, state_ent_coef=1.0, latent_ent_coef=1.0,
                               latent_cond_ent_coef=1.0, update_encoder=True, **kw)
    return agents.ProtoAgent(pred_dim=32, proj_dim=64, queue_size=256, num_protos=32, tau=0.1, encoder_target_tau=0.05, topk=3,
                             update_encoder=True, **kw)


def arena(kind, obs_type, seed=5):
    """An ArenaIterator with the Philox sampler over synthetic episodes: the loader's sample_into branch."""
    import _synth
    from exorl_amd.engine import ReplayEngine
    from exorl_amd.replay_buffer import ArenaIterator
    pix = obs_type == 'pixels'
    M = META[obs_type].get(kind, 0)
    shape, rows, batch = ((PC, PHW, PHW), 60, PB) if pix else ((O,), 300, B)
    eps = _synth.synth_episodes(seed, [rows] * 3, int(np.prod(shape)), A, M, obs_u8=pix)
    eng = ReplayEngine(shape, np.uint8 if pix else np.float32, A, M, 3 * (rows + 1) + 64, 16, 'cuda:0')
    eng.set_order([eng.append_episode(ep, ('skill',) if M else ()) for ep in eps])
    eng.seed_philox(seed)
    return ArenaIterator(eng, batch, 1 if kind in OFFLINE + OFFLINE_LATER else 3, 0.99, 'philox')


def bind_prdc(ag, it, seed=5):
    """PRDC's key table, built from a small arena and bound, as tests/_prdc_cases.bind does: the arena `it` samples from when it is an
    ArenaIterator, else one of its own (a plain iterator of batches has no dataset). Returns what must stay alive while the agent steps; a
    no-op for every other class."""
    if ag.KIND != 'prdc':
        return None
    table = it if hasattr(it, '_arenas') else arena('prdc', 'states', seed)
    assert ag.bind_dataset(table) == 900
    return table


def batches(kind, obs_type, first, n):
    """A plain iterator of 5- or 6-tuples: the loader's next() branch."""
    import _synth
    pix = obs_type == 'pixels'
    M = META[obs_type].get(kind, 0)
    for step in range(first, first + n):
        rs = np.random.RandomState(900 + step)
        if pix:
            frames = [rs.randint(0, 256, (PB, PC, PHW, PHW)).astype(np.uint8) for _ in range(2)]
            _, act, rew, disc, _ = _synth.synth_batch(41, step, PB, 4, A)
            b = [frames[0], act, rew, disc, frames[1]]
        else:
            b = list(_synth.synth_batch(41, step, B, O, A))
        if M:
            m = rs.standard_normal((b[1].shape[0], M)).astype(np.float32)
            b.append(m / np.linalg.norm(m, axis=1, keepdims=True) if kind == 'aps' else np.eye(M, dtype=np.float32)[m.argmax(1)])
        yield tuple(b)


def set_hooks(ag, seed):
    """Every hook an agent has, all fed from ONE stream: a changed call order changes every later draw."""
    rs = np.random.RandomState(seed)
    normal = lambda shape: rs.standard_normal(tuple(shape)).astype(np.float32)
    ag.noise_hook = lambda shape, dist='normal': np.tanh(normal(shape)) if dist == 'uniform' else normal(shape)
    if hasattr(ag, 'shift_hook'):
        ag.shift_hook = lambda n: rs.randint(0, 9, (n, 2)).astype(np.int32)
    if hasattr(ag, 'cat_hook'):
        ag.cat_hook = lambda n: rs.uniform(size=n).astype(np.float32)
    if hasattr(ag, 'eps_hook'):
        ag.eps_hook = normal


def digest(ag, emit):
    """Everything that defines the agent's state, one entry each."""
    import torch
    from exorl_amd import _lib as L
    torch.cuda.synchronize()
    eng = ag.engine
    emit('engine.workspace', sha(eng.workspace))
    if getattr(ag, 'obs_type', 'states') == 'pixels':
        st = eng.export_state()
        emit('engine.steps', sha(st['steps'])), emit('engine.counters', sha(st['counters'])), emit('engine.bn2d', sha(st['bn2d']))
        for (net, what), ts in sorted(st['tensors'].items()):
            emit(f'engine.net{net}.what{what}', sha(torch.cat([t.reshape(-1) for t in ts])))
        for i, t in enumerate(st['enc_extra']):
            emit(f'engine.enc_extra{i}', sha(t))
        for name in ('encoder', 'actor', 'critic'):
            emit(f'engine.{name}.grads', sha(torch.cat([g.reshape(-1) for g in getattr(ag, name).grads()])))
    else:
        for net in [L.NET_ACTOR] + ([L.NET_CRITIC, L.NET_CRITIC_TARGET] if eng.has_critic else []) + ([L.NET_VALUE] if getattr(eng, 'has_value', False) else []):
            for what in ((L.T_PARAM,) if net == L.NET_CRITIC_TARGET else (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V, L.T_GRAD)):
                emit(f'engine.net{net}.what{what}', sha(eng.flat(net, what)))
            for name, image in eng.weight_images(net).items():      # the derived weight copies one by one: a differing workspace digest gets a name
                if image is not None:
                    emit(f'engine.net{net}.image.{name}', sha(image))
        emit('engine.opt_steps', sha(repr(eng.opt_steps()))), emit('engine.noise_counter', sha(repr(eng.noise_counter())))
        if ag.KIND == 'cql':
            emit('engine.cql_alpha', sha(eng.cql_alpha_state()))
    if hasattr(ag, 'intr'):
        it = ag.intr
        emit('intr.workspace', sha(it.workspace))
        for what in (L.T_PARAM, L.T_ADAM_M, L.T_ADAM_V, L.T_GRAD):
            emit(f'intr.what{what}', sha(it.flat(what)))
        emit('intr.rms', sha(it._rms)), emit('intr.opt_steps', sha(repr(it.opt_steps()))), emit('intr.counter', sha(repr(it.counter())))
        if it.bn is not None:
            emit('intr.bn', sha(it.bn))
        if it.queue is not None:
            emit('intr.queue', sha(it.queue)), emit('intr.queue_ptr', sha(repr(it.queue_ptr())))
    for name in ('encoder_target', 'rnd_target_encoder', 'rnd', 'predictor_target'):       # views that add buffers or sit outside the net table
        view = getattr(ag, name, None)
        if hasattr(view, 'state_dict'):
            emit(f'{name}.state_dict', sha(','.join(f'{k}={sha(v)}' for k, v in view.state_dict().items())))
    from exorl_amd import snapshot
    st = ag.__getstate__()
    emit('getstate.attrs', sha(','.join(sorted(st['attrs']))))
    emit('getstate.keys', sha(','.join(list(st) + [f'intr.{k}' for k in st.get('intr', ())])))      # the pickled dict's layout, in its order
    emit('snapshot.names', sha(','.join(snapshot.state_dicts(ag))))
    emit('surface.public', sha(','.join(n for n in dir(ag) if not n.startswith('_') and hasattr(ag, n))))


def emit_metrics(emit, tag, m):
    emit(f'{tag}.keys', sha(','.join(sorted(m))))
    for k in sorted(m):
        emit(f'{tag}.{k}', float(m[k]).hex())


def act_inputs(ag, kind, obs_type):
    rs = np.random.RandomState(77)
    obs = rs.randint(0, 256, (PC, PHW, PHW)).astype(np.uint8) if obs_type == 'pixels' else rs.standard_normal(O).astype(np.float32)
    if kind in OFFLINE + OFFLINE_LATER:
        return (obs,)
    M = META[obs_type].get(kind, 0)
    meta = {'m': np.eye(M, dtype=np.float32)[1]} if M else {}
    return (obs, meta)


def run_case(emit, kind, obs_type, reward_free, precision, mode, first, n, ag=None, use_tb=True):
    """`n` update() calls from step `first` over an ArenaIterator without hooks (mode 'arena'), a plain iterator with every hook set
    ('hooks'), or a captured graph ('graph'); then the digests and one act() in each mode."""
    ag = ag or build(kind, obs_type, reward_free, precision, use_tb)
    if not hasattr(ag, 'num_expl_steps'):
        ag.num_expl_steps = 0              # the offline classes leave it to the training script; act() reads it
    if mode == 'hooks':
        set_hooks(ag, 100 + first)
        it = batches(kind, obs_type, first, n)
    else:
        it = arena(kind, obs_type, 5 + first)
    table = bind_prdc(ag, it, 5 + first)       # an unpickled agent (part2) binds again: the table is the arena's, not the agent's
    if mode == 'graph':
        assert ag.enable_graph(it)
    for i in range(first, first + n):
        emit_metrics(emit, f'metrics{i}', ag.update(it, i))
    digest(ag, emit)
    for eval_mode in (True, False):
        emit(f'act.eval{int(eval_mode)}', sha(np.asarray(ag.act(*act_inputs(ag, kind, obs_type), 10, eval_mode), np.float32)))
    del table
    return ag


def cases():
    """(name, kind, obs_type, reward_free, precision, mode, use_tb) of every case."""
    def case(kind, obs_type, reward_free, precision, mode, use_tb=True):
        name = f'{obs_type}/{kind}/{"pretrain" if reward_free else "finetune"}/{precision}/{mode}' + ('' if use_tb else '/no_tb')
        return name, kind, obs_type, reward_free, precision, mode, use_tb
    for mode in ('arena', 'hooks'):
        for precision in PRECISIONS['states']:
            for kind in OFFLINE:
                yield case(kind, 'states', False, precision, mode)
        for obs_type in ('states', 'pixels'):
            for precision in PRECISIONS[obs_type]:
                for kind in ['ddpg'] + MODULES:
                    for reward_free in (True, False):
                        yield case(kind, obs_type, reward_free, precision, mode)
    yield case('td3_bc', 'states', False, 'bf16x3', 'graph', use_tb=False)
    yield case('smm', 'states', True, 'fp32', 'hooks', use_tb=False)     # SMM reports its module's metrics whatever use_tb says
    for kind in OFFLINE_LATER:
        for mode in ('arena', 'hooks'):
            for precision in PRECISIONS['states']:
                yield case(kind, 'states', False, precision, mode)
        yield case(kind, 'states', False, 'bf16x3', 'graph', use_tb=False)


def listing(path, body):
    import torch
    if not torch.cuda.is_available():
        sys.exit('agent_digests: needs a GPU')
    lines = []
    body(lambda case: (lambda what, value: lines.append(f'{case} {what} {value}')))
    Path(path).write_text('\n'.join(lines) + '\n')
    print(f'{path}: {len(lines)} entries')


def part1(out, pickle_dir=None):
    def body(emitter):
        for name, *c, use_tb in cases():
            ag = run_case(emitter(name), *c, 0, 3, use_tb=use_tb)
            if pickle_dir:
                if c[-1] == 'graph':
                    ag.disable_graph()
                Path(pickle_dir, name.replace('/', '__') + '.pkl').write_bytes(pickle.dumps(ag))
            print(name, flush=True)
    if pickle_dir:
        Path(pickle_dir).mkdir(parents=True, exist_ok=True)
    listing(out, body)


def part2(out, pickle_dir):
    def body(emitter):
        for name, *c, use_tb in cases():
            ag = pickle.loads(Path(pickle_dir, name.replace('/', '__') + '.pkl').read_bytes())
            run_case(emitter(name), *c, 3, 1, ag=ag)
            print(name, flush=True)
    listing(out, body)


WORKERS = ['_dp_worker.py', '_pixel_dp_worker.py', '_pixel_module_dp_worker.py', '_proto_pixel_dp_worker.py', '_state_module_dp_worker.py']


def part3(out):
    """Each worker script as its test fixture starts it: two fresh rank processes on cuda:0 over gloo."""
    def body(emitter):
        for worker in WORKERS:
            tmp = Path(tempfile.mkdtemp(prefix='agent_digests_'))
            args = [str(tmp)]
            if worker == '_dp_worker.py':
                import _dp_worker
                _dp_worker.write_dataset(tmp / 'buffer')
                (tmp / 'out').mkdir()
                args = [str(tmp / 'buffer'), str(tmp / 'out')]
            with socket.socket() as s:
                s.bind(('127.0.0.1', 0))
                port = s.getsockname()[1]
            procs = []
            for rank in range(2):
                env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
                procs.append(subprocess.Popen([sys.executable, str(ROOT / 'tests' / worker), *args], env=env,
                                              stdout=open(tmp / f'rank{rank}.log', 'w'), stderr=subprocess.STDOUT))
            try:
                rcs = [p.wait(timeout=600) for p in procs]
            finally:
                for p in procs:
                    if p.poll() is None:
                        p.kill()
            if any(rcs):
                sys.exit(f'{worker}: exit status {rcs}\n' + ''.join((tmp / f'rank{r}.log').read_text()[-3000:] for r in range(2)))
            emit = emitter(worker)
            for f in sorted(tmp.rglob('*.npz')):
                if 'buffer' in f.relative_to(tmp).parts:
                    continue
                z = np.load(f, allow_pickle=False)
                for k in sorted(z.files):
                    emit(f'{f.name}:{k}', sha(z[k]))
            for f in sorted(tmp.rglob('*.json')):
                emit(f.name, sha(json.dumps(json.load(open(f)), sort_keys=True)))
            print(worker, flush=True)
    listing(out, body)


def grid(out):
    """tests/_grad_grid.CASES and tests/_state_bf16x6_cases.CASES on the three routes of tests/test_gpu_grad_grid.py: one update() as its run()
    does it, then every tensor of its state_of(). Behind them tests/_prdc_cases.CASES on the two routes of tests/test_gpu_prdc.py, likewise."""
    import _grad_grid as G
    import _prdc_cases as P
    import _state_bf16x6_cases as S
    import test_gpu_grad_grid as T
    import test_gpu_prdc as TP

    def body(emitter):
        for c in list(G.CASES) + list(S.CASES):
            for route in T.ROUTES:
                name = f'grid/{G.case_id(c)}/{route}'
                ag, m = T.run(c, route, False)
                emit = emitter(name)
                emit_metrics(emit, 'metrics', m)
                for k, v in T.state_of(ag).items():
                    emit(k, sha(v))
                print(name, flush=True)
        for c in P.CASES:
            for route in ('metrics', 'fast'):
                name = f'grid/{P.case_id(c)}/{route}'
                ag, m, keep = TP.run(c, route)
                emit = emitter(name)
                emit_metrics(emit, 'metrics', m)
                for k, v in TP.state_of(ag).items():
                    emit(k, sha(v))
                del keep
                print(name, flush=True)
    listing(out, body)


def modes(out):
    """TD3+BC, CQL, IQL, FQE and PRDC, one handle each per precision and metrics setting, driven in turn by a captured graph step, disable_graph,
    the phased calls, an eager update() and a newly captured graph step, with the digests after every driver: what one driver sets up for
    its own launches (fused optimiser and scalar-head kernels, staged inputs, capture) must not reach the next one's. TD3+BC and CQL run
    phases 0..3 and use only calls that trees from before exorl_agent_update_plan have; IQL, FQE and PRDC (no metric window) run the phase
    ids of their own plan, as AgentEngine.update_steps reads it; PRDC searches the table of the arena it samples from."""
    def plan_phases(eng):
        import ctypes as C
        from exorl_amd import _lib as L
        phases, xids, n = (C.c_int32 * 8)(), (C.c_int32 * 8)(), C.c_int32()
        L.check(eng.lib.exorl_agent_update_plan(C.byref(eng.cfg), phases, xids, 8, C.byref(n)))
        return list(phases[:n.value])

    def body(emitter):
        for kind in ['td3_bc', 'cql'] + OFFLINE_LATER:
            for precision in ('fp32', 'bf16x3'):
                for metrics in ('tb', 'no_tb') + (('window',) if kind not in OFFLINE_LATER else ()):
                    name = f'modes/{kind}/{precision}/{metrics}'
                    emit = emitter(name)
                    ag = build(kind, 'states', False, precision, metrics == 'tb')
                    if metrics == 'window':
                        assert ag.enable_metric_window()
                    it = arena(kind, 'states')
                    bind_prdc(ag, it)
                    stddev = 1.0 if kind == 'cql' else ag._stddev(0)

                    def after(tag):
                        emit(f'{tag}.metrics_raw', sha(ag.engine.metrics_raw()))
                        digest(ag, lambda what, value: emit(f'{tag}.{what}', value))
                    assert ag.enable_graph(it)
                    emit_metrics(emit, 'graph0', ag.update(it, 0))
                    after('graph0')
                    ag.disable_graph()
                    ag._load_batch(it)
                    for phase in (plan_phases(ag.engine) if kind in OFFLINE_LATER else range(4)):
                        ag.engine.update_phase(phase, stddev)
                    after('phased')
                    emit_metrics(emit, 'eager', ag.update(it, 2))
                    after('eager')
                    assert ag.enable_graph(it)
                    emit_metrics(emit, 'graph1', ag.update(it, 3))
                    after('graph1')
                    if metrics == 'window':
                        sums, steps = ag.engine.metric_window_read(reset=False)
                        emit('window.sums', sha(sums)), emit('window.steps', str(steps))
                    ag.disable_graph()
                    print(name, flush=True)
    listing(out, body)


def pixel_modes(out):
    """Plain DDPG and ICM on pixels, one handle each per precision, driven in turn by the three phased calls, a one-call update(), a
    one-call step on kept images, one on kept encodings and a one-call update() again, with the digests after every driver: what one call
    decides for its own launches (image mode, phase, communicator) must not reach the next one's. Uses only calls that trees from before
    exorl_pixel_step have, so the same file runs against either library."""
    def body(emitter):
        for kind in ('ddpg', 'icm'):
            for precision in PRECISIONS['pixels']:
                name = f'pixel_modes/{kind}/{precision}'
                emit = emitter(name)
                ag = build(kind, 'pixels', True, precision)
                eng, it, stddev = ag.engine, arena(kind, 'pixels'), ag._stddev(0)

                def after(tag):
                    emit(f'{tag}.metrics_raw', sha(eng.metrics_raw()))
                    digest(ag, lambda what, value: emit(f'{tag}.{what}', value))
                ag._load_batch(it)
                images = ag._pix_before_step()          # ICM: its module and encoder step, then keep_encoded
                eng.update_phase(0, stddev, **images)
                eng.update_phase(1, stddev)
                eng.update_phase(2, stddev)
                ag._pix_after_step()
                after('phased')
                emit_metrics(emit, 'one_call', ag.update(it, 1))
                after('one_call')
                ag._load_batch(it)
                eng.augment()
                eng.update(stddev, keep_augmented=True)
                after('keep_augmented')
                ag._load_batch(it)
                eng.augment()
                eng.encode(0), eng.encode(1)
                eng.set_train_encoder(False)
                eng.update(stddev, keep_encoded=True)
                eng.set_train_encoder(kind == 'ddpg')
                after('keep_encoded')
                emit_metrics(emit, 'one_call_again', ag.update(it, 4))
                after('one_call_again')
                print(name, flush=True)
    listing(out, body)


REPLAY_LENGTHS = [5, 9, 3, 12, 7, 4]


def replay(out):
    """The replay loaders, first three batches of 16 each: every output tensor and the (episode, start) pairs of every arena call behind
    it (ReplayEngine.last_pairs). Online loaders (MT19937 with fetch_every below the batch, so a batch is split where the reference would
    re-scan; Philox with two workers) over states with one 4-wide meta spec; offline loaders over one directory, two mixed ones under both
    weightings, stacked uint8 frames, normalize_obs on two shards, and a hold-out split with its hold-out iterator and its training
    arena behind an ArenaIterator. Uses only calls that trees from before ReplayEngine.alloc_batch have,
    so the same file runs against either library."""
    import random
    import _synth
    from exorl_amd import replay_buffer as R
    from exorl_amd.engine import ReplayEngine
    NB, RB, K = 3, 16, 3

    class Spec:
        def __init__(self, shape, dtype, name):
            self.shape, self.dtype, self.name = tuple(shape), np.dtype(dtype), name

    pairs, inner = [], ReplayEngine.sample_into

    def sample_into(self, out_, batch, *a, **k):            # every arena call of a batch, in order: a split batch makes several
        r = inner(self, out_, batch, *a, **k)
        pairs.append(self.last_pairs(batch))
        return r
    ReplayEngine.sample_into = sample_into

    def record(emit, tag, it, nb=NB):
        for bi in range(nb):
            del pairs[:]
            for ti, t in enumerate(next(it)):
                emit(f'{tag}{bi}.t{ti}', sha(t))
            emit(f'{tag}{bi}.pairs', sha(np.concatenate(pairs)))

    def states(seed, lengths=REPLAY_LENGTHS, meta=0):
        return _synth.synth_episodes(seed, lengths, O, A, meta)

    def frames(seed):
        eps = _synth.synth_episodes(seed, REPLAY_LENGTHS, 3 * 8 * 8, A, obs_u8=True)
        return [dict(ep, observation=R.stack_frames(ep['observation'].reshape(-1, 3, 8, 8), K)) for ep in eps]

    def write(tmp, name, eps):
        d = tmp / name
        d.mkdir()
        for i, ep in enumerate(eps):
            R.save_episode(ep, d / f'episode_{i}_{R.episode_len(ep)}.npz')
        return d

    def online(tmp, **kw):
        st = R.ReplayBufferStorage((), (Spec((4,), np.float32, 'skill'),), tmp / 'buffer')
        for ep in states(21, meta=4):
            st._store_episode(ep)
        random.seed(3), np.random.seed(3)
        return iter(R.make_replay_loader(st, 10**6, RB, kw.pop('num_workers', 0), True, 3, 0.99, **kw))

    def offline(dirs, **kw):
        random.seed(3), np.random.seed(3)
        kw.setdefault('sampler', 'philox'), kw.setdefault('seed', 4)
        return iter(R.make_offline_replay_loader(None, dirs, 10**6, RB, kw.pop('num_workers', 1), 0.99, **kw))

    def body(emitter):
        def case(name, run):
            with tempfile.TemporaryDirectory(prefix='agent_digests_') as tmp:
                run(emitter(f'replay/{name}'), Path(tmp))
            print(name, flush=True)
        case('online/mt19937/segments', lambda emit, tmp: record(emit, 'batch', online(tmp, fetch_every=5)))
        case('online/philox/workers', lambda emit, tmp: record(emit, 'batch', online(tmp, num_workers=2, sampler='philox', seed=11,
                                                                                     worker_ids=[0, 1])))
        case('offline/one_dir', lambda emit, tmp: record(emit, 'batch', offline(write(tmp, 'a', states(22)))))
        case('offline/one_dir/mt19937', lambda emit, tmp: record(emit, 'batch', offline(write(tmp, 'a', states(22)), sampler='mt19937',
                                                                                       seed=None)))
        for weighting in ('episodes', 'transitions'):
            case(f'offline/mix/{weighting}', lambda emit, tmp: record(emit, 'batch', offline(
                [write(tmp, 'a', states(22)), write(tmp, 'b', states(23, REPLAY_LENGTHS[::-1]))], mix=[0.75, 0.25], weighting=weighting)))
        case('offline/frame_stack', lambda emit, tmp: record(emit, 'batch', offline(write(tmp, 'a', frames(24)), frame_stack=K)))

        def normalized(emit, tmp):
            it = offline(write(tmp, 'a', states(22)), num_workers=2, normalize_obs=True)
            record(emit, 'batch', it)
            emit('obs_normalizer', sha(np.concatenate([np.asarray(x, np.float32).reshape(-1) for x in it.obs_normalizer])))
        case('offline/normalize_obs/two_shards', normalized)

        def holdout(emit, tmp):
            it = offline(write(tmp, 'a', states(22)), holdout_every=2)
            record(emit, 'batch', it)
            record(emit, 'holdout', it.holdout)
            record(emit, 'arena', R.ArenaIterator(it.engine, RB, 1, 0.99, 'philox'))
            emit('files', sha(','.join(fn.name for sh in it.shards for fn in [*sh.fns, *sh.holdout_fns])))
        case('offline/holdout', holdout)
    try:
        listing(out, body)
    finally:
        ReplayEngine.sample_into = inner


def compare(a, b):
    la, lb = Path(a).read_text().splitlines(), Path(b).read_text().splitlines()
    key = lambda l: l.rsplit(' ', 1)[0]
    da, db = {key(l): l for l in la}, {key(l): l for l in lb}
    diff = [f'{da.get(k, k + " <missing>")}  |  {db.get(k, "<missing>").rsplit(" ", 1)[-1]}' for k in sorted(set(da) | set(db))
            if da.get(k) != db.get(k)]
    print(f'{len(set(da) | set(db))} entries, {len(diff)} differ')
    for d in diff:
        print(d)
    return 1 if diff else 0


def summary(a, b):
    """One line per case of two listings, in listing order: case | entries | lines digest and engine.workspace of each. The lines digest is
    the md5 of the case's `what value` lines joined by newlines."""
    def table(path):
        cases = {}
        for line in Path(path).read_text().splitlines():
            case, rest = line.split(' ', 1)
            cases.setdefault(case, []).append(rest)
        return cases

    def cell(lines):
        ws = [l.rsplit(' ', 1)[1] for l in lines if l.split(' ')[0].endswith('engine.workspace')]
        return f"{hashlib.md5(chr(10).join(lines).encode()).hexdigest()} {ws[-1] if ws else '-'}"
    ta, tb = table(a), table(b)
    for path in (a, b):
        print(f'# {path}: sha256 {hashlib.sha256(Path(path).read_bytes()).hexdigest()}, {Path(path).stat().st_size} bytes')
    print('Columns: case | entries | parent: lines digest, engine.workspace | this tree: lines digest, engine.workspace')
    for case in ta:
        print(f"{case} | {len(ta[case])} | {cell(ta[case])} | {cell(tb.get(case, []))}")
    return 0


if __name__ == '__main__':
    cmd, args = sys.argv[1], sys.argv[2:]
    sys.exit({'part1': part1, 'part2': part2, 'part3': part3, 'grid': grid, 'modes': modes, 'pixel_modes': pixel_modes, 'replay': replay, 'compare': compare, 'summary': summary}[cmd](*args))
