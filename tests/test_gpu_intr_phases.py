"""The exchanges that exorl_intr_update_phase names, phase by phase until -1, for every kind of module, `train`, world size and the
configuration flags that change them, against a literal table. The table is what the recorder below gave on the commit before the steps
became one plan per kind and one driver (profiles/intr_stages_sequences.txt holds that listing and this tree's); 'raises' stands for a
refused first phase. One phase past the end of a sequence is refused in every case.

World size 2 is two engines in this process whose exchanges are performed here in rank order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ['rnd', 'icm', 'icm_apt', 'disagreement', 'diayn', 'aps', 'smm', 'proto']
O, A, H, R, B, K = 12, 4, 64, 16, 32, 3          # B rows per rank; R also the width of the skill / task / z columns behind the observation
GRAD, REP, MOMENTS, BN = 0, 1, 2, 3              # EXORL_INTR_XCHG_*


def _cases():
    """(kind, train, world, flag): flag is '', 'encoded' or 'no_rms'."""
    for world in (1, 2):
        for kind in KINDS:
            for train in (1, 0):
                yield kind, train, world, ''
        yield 'proto', 2, world, ''
        for kind in ('rnd', 'smm'):
            for train in (1, 0) + ((2,) if kind == 'rnd' else ()):
                yield kind, train, world, 'encoded'
        for kind in ('icm_apt', 'aps'):
            for train in (1, 0):
                yield kind, train, world, 'no_rms'
    yield 'rnd', 2, 1, ''                        # the step-only call on state rows
    yield 'rnd', 2, 2, ''


CASES = list(_cases())
RAISES = 'raises'
# (kind, train, world, flag) -> the ids named by phases 0, 1, ... of one step
TABLE = {
    ('rnd', 1, 1, ''): [GRAD, -1],
    ('rnd', 0, 1, ''): [-1],
    ('icm', 1, 1, ''): [GRAD, -1],
    ('icm', 0, 1, ''): [-1],
    ('icm_apt', 1, 1, ''): [GRAD, -1],
    ('icm_apt', 0, 1, ''): [-1],
    ('disagreement', 1, 1, ''): [GRAD, -1],
    ('disagreement', 0, 1, ''): [-1],
    ('diayn', 1, 1, ''): [GRAD, -1],
    ('diayn', 0, 1, ''): [-1],
    ('aps', 1, 1, ''): [GRAD, -1],
    ('aps', 0, 1, ''): [-1],
    ('smm', 1, 1, ''): [GRAD, -1],
    ('smm', 0, 1, ''): RAISES,
    ('proto', 1, 1, ''): [GRAD, -1],
    ('proto', 0, 1, ''): [-1],
    ('proto', 2, 1, ''): [GRAD, -1],
    ('rnd', 1, 1, 'encoded'): [GRAD, -1],
    ('rnd', 0, 1, 'encoded'): [-1],
    ('rnd', 2, 1, 'encoded'): [GRAD, -1],
    ('smm', 1, 1, 'encoded'): [GRAD, -1],
    ('smm', 0, 1, 'encoded'): RAISES,
    ('icm_apt', 1, 1, 'no_rms'): [GRAD, -1],
    ('icm_apt', 0, 1, 'no_rms'): [-1],
    ('aps', 1, 1, 'no_rms'): [GRAD, -1],
    ('aps', 0, 1, 'no_rms'): [-1],
    ('rnd', 1, 2, ''): [BN, GRAD, MOMENTS, -1],
    ('rnd', 0, 2, ''): [BN, MOMENTS, -1],
    ('icm', 1, 2, ''): [GRAD, -1],
    ('icm', 0, 2, ''): [-1],
    ('icm_apt', 1, 2, ''): [GRAD, REP, MOMENTS, -1],
    ('icm_apt', 0, 2, ''): [REP, MOMENTS, -1],
    ('disagreement', 1, 2, ''): [GRAD, -1],
    ('disagreement', 0, 2, ''): [-1],
    ('diayn', 1, 2, ''): [GRAD, -1],
    ('diayn', 0, 2, ''): [-1],
    ('aps', 1, 2, ''): [GRAD, REP, MOMENTS, -1],
    ('aps', 0, 2, ''): [REP, MOMENTS, -1],
    ('smm', 1, 2, ''): [GRAD, MOMENTS, -1],
    ('smm', 0, 2, ''): RAISES,
    ('proto', 1, 2, ''): [REP, GRAD, REP, -1],
    ('proto', 0, 2, ''): [REP, -1],
    ('proto', 2, 2, ''): [REP, GRAD, -1],
    ('rnd', 1, 2, 'encoded'): [GRAD, MOMENTS, -1],
    ('rnd', 0, 2, 'encoded'): [MOMENTS, -1],
    ('rnd', 2, 2, 'encoded'): [GRAD, -1],
    ('smm', 1, 2, 'encoded'): [GRAD, -1],
    ('smm', 0, 2, 'encoded'): RAISES,
    ('icm_apt', 1, 2, 'no_rms'): [GRAD, REP, -1],
    ('icm_apt', 0, 2, 'no_rms'): [REP, -1],
    ('aps', 1, 2, 'no_rms'): [GRAD, REP, -1],
    ('aps', 0, 2, 'no_rms'): [REP, -1],
    ('rnd', 2, 1, ''): RAISES,
    ('rnd', 2, 2, ''): RAISES,
}


def case_id(c):
    kind, train, world, flag = c
    return f'{kind}-train{train}-world{world}' + (f'-{flag}' if flag else '')


def _ranks(kind, world, flag):
    from exorl_amd.engine import IntrEngine
    kw = dict(rep_dim=R, lr=1e-4, precision='fp32', knn_k=K, knn_avg=True, knn_rms=flag != 'no_rms', knn_clip=0.0, encoded=flag == 'encoded')
    if kind == 'disagreement':
        kw['n_models'] = 5
    if kind == 'proto':
        kw.update(num_protos=16, queue_size=80)
    ranks = [IntrEngine(kind, O, A, H, B, world_size=world, rank=r, **kw) for r in range(world)]
    for m in ranks:
        p = m.flat()
        p.copy_((torch.randn(p.numel(), generator=torch.Generator().manual_seed(17)) * 0.05).to(p.device))
    return ranks


def _args(kind, rank, train):
    """One rank's rows as [obs | meta]; every kind reads what it needs of them."""
    rs = np.random.RandomState(40 + rank)
    meta = np.eye(R, dtype=np.float32)[rs.randint(0, R, B)]
    t = dict(obs=np.concatenate([rs.standard_normal((B, O)).astype(np.float32), meta], 1),
             next_obs=np.concatenate([rs.standard_normal((B, O)).astype(np.float32), meta], 1),
             action=rs.uniform(-1, 1, (B, A)).astype(np.float32), reward=rs.uniform(0, 1, B).astype(np.float32),
             u=rs.uniform(0, 1, 128 * B).astype(np.float32))
    t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    p = {k: v.data_ptr() for k, v in t.items()}
    kw = dict(skill=p['obs'] + 4 * O, obs_ld=O + R, next_obs_ld=O + R, skill_ld=O + R, cat_uniform=p['u'])
    return t, (p['obs'], p['action'], p['next_obs'], p['reward'], p['reward'], train), kw


def _exchange(ranks, xid):
    """What the collective does across the ranks: the sum, or every rank's slot into every rank's buffer."""
    from exorl_amd import _lib as L
    bufs = [m.exchange(xid) for m in ranks]
    assert len({op for _, op in bufs}) == 1
    if bufs[0][1] == L.XCHG_SUM:
        total = sum(b for b, _ in bufs)
        for b, _ in bufs:
            b.copy_(total)
    else:
        for src, (b, _) in enumerate(bufs):
            for dst, _ in bufs:
                dst[src].copy_(b[src])


def record(case, past_end=True):
    """The ids one step names, phase by phase, or RAISES when the first phase is refused; then, if asked for, whether one phase past the
    end is refused (the commit the table comes from did not refuse every one, so its listing was recorded without)."""
    from exorl_amd._lib import ExorlError
    kind, train, world, flag = case
    ranks = _ranks(kind, world, flag)
    calls = [_args(kind, r, train) for r in range(world)]          # keeps the rows alive
    seen, phase = [], 0
    try:
        while not seen or seen[-1] >= 0:
            nxt = {m.update_phase(phase, *a, **kw) for m, (_, a, kw) in zip(ranks, calls)}
            assert len(nxt) == 1, nxt
            seen.append(nxt.pop())
            if seen[-1] >= 0:
                _exchange(ranks, seen[-1])
            phase += 1
    except ExorlError:
        assert not seen, (case, seen)
        torch.cuda.synchronize()
        return RAISES, True
    if past_end:
        with pytest.raises(ExorlError, match=r'intr_update_phase: phase \d+ out of range'):
            ranks[0].update_phase(phase, *calls[0][1], **calls[0][2])
    torch.cuda.synchronize()
    return seen, past_end


def test_the_table_covers_every_case():
    assert sorted(TABLE) == sorted(CASES) and len(set(CASES)) == len(CASES)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_update_phase_names_the_exchanges_of_the_table(case):
    seen, _ = record(case)
    print(case_id(case), seen)
    assert seen == TABLE[case]
