"""The pixel step's drivers through PixelEngine's Python surface: every phased call names the exchange behind each phase, the three image
modes (fresh augmentation, kept images, kept encodings) are one step, nothing of one driver call reaches the next, and what cannot be a
step is refused. One process, no process group: nothing is exchanged, the buffers are only named."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_pixel_dp import _batch, _engine, _set, _shifts

pytestmark = pytest.mark.gpu

C_, HW, A, F, H, B = 3, 64, 6, 32, 128, 32
STDDEV = 0.2


def _pair(precision='fp32'):
    return [_engine(C_, HW, A, F, H, B, precision=precision) for _ in range(2)]


def _draws(seed):
    rs = np.random.RandomState(seed)
    return _shifts(rs, B), _shifts(rs, B), rs.standard_normal((B, A)).astype(np.float32), rs.standard_normal((B, A)).astype(np.float32)


def _assert_same_step(x, y, what):
    sx, sy = x.export_state(), y.export_state()
    assert np.array_equal(sx['steps'], sy['steps']) and np.array_equal(sx['counters'], sy['counters']), what
    assert sx['tensors'].keys() == sy['tensors'].keys()
    for k in sx['tensors']:
        for i, (tx, ty) in enumerate(zip(sx['tensors'][k], sy['tensors'][k])):
            assert torch.equal(tx, ty), (what, k, i)
    assert torch.equal(sx['bn2d'], sy['bn2d']), what
    for i, (tx, ty) in enumerate(zip(sx['enc_extra'], sy['enc_extra'])):
        assert torch.equal(tx, ty), (what, 'enc_extra', i)
    assert np.array_equal(x.metrics_raw(), y.metrics_raw()), what


def _walk(steps):
    """The (data_ptr, numel, dtype, op) of every exchange a *_steps generator yields, exchanging nothing, and what the call returns."""
    seen = []
    while True:
        try:
            buf, op = next(steps)
        except StopIteration as done:
            return seen, done.value
        seen.append((buf.data_ptr(), buf.numel(), buf.dtype, op))


def _named(e, xid):
    buf, op = e.exchange(xid)
    return buf.data_ptr(), buf.numel(), buf.dtype, op


# ---------------------------------------------------------------------------------------------------- 1. phases name their exchanges
def test_phases_name_their_exchanges():
    from exorl_amd import _lib as L
    e = _engine(C_, HW, A, F, H, B)
    _set(e, _batch(3, B, C_, HW, A))
    enc_total = e.grad_buffer(2).numel()
    e.set_train_encoder(False)
    critic_total = e.grad_buffer(0).numel()
    steps = e.export_state()['steps'].copy()
    for train, total in ((True, critic_total + enc_total), (False, critic_total)):
        e.set_train_encoder(train)
        seen, _ = _walk(e.update_steps(STDDEV))
        assert seen == [_named(e, 0), _named(e, 1)], train
        assert seen[0] == (e.grad_buffer(0).data_ptr(), total, torch.float32, L.XCHG_SUM), train
        assert seen[1] == (e.grad_buffer(1).data_ptr(), e.grad_buffer(1).numel(), torch.float32, L.XCHG_SUM), train
        steps += np.array([1, 0, int(train)])               # critic_opt / actor_opt, proto_opt's encoder state, encoder_opt
        assert np.array_equal(e.export_state()['steps'], steps), train
    e.augment()
    dfeat = torch.randn_like(e.feature_view(e.encode(0)))
    seen, _ = _walk(e.encoder_step_steps(0, dfeat.data_ptr(), 0))
    assert seen == [_named(e, 2)] == [(e.grad_buffer(2).data_ptr(), enc_total, torch.float32, L.XCHG_SUM)]
    steps += np.array([0, 0, 1])
    assert np.array_equal(e.export_state()['steps'], steps)
    seen, feats = _walk(e.rnd_features_steps())
    assert seen == [_named(e, 3)] * 2 == [(e.bn_partials().data_ptr(), C_ * 128, torch.float64, L.XCHG_SUM)] * 2
    assert len(feats) == 2 and all(feats) and feats[0] != feats[1]
    assert np.array_equal(e.export_state()['steps'], steps)


# ---------------------------------------------------------------------------------------------------- 2. the image modes are one step
@pytest.mark.parametrize('precision', ['fp32', 'bf16x6'])
def test_image_modes_are_the_same_step(precision):
    x, y = _pair(precision)
    for e in (x, y):
        _set(e, _batch(11, B, C_, HW, A))
    so, sn, nc, na = _draws(21)
    x.update(STDDEV, so, sn, nc, na)
    y.augment(so, sn)
    y.update(STDDEV, noise_critic=nc, noise_actor=na, keep_augmented=True)
    _assert_same_step(x, y, 'fresh with given shifts vs augment + keep_augmented')
    for e in (x, y):
        _set(e, _batch(12, B, C_, HW, A))
        e.set_train_encoder(False)
    so, sn, nc, na = _draws(22)
    x.update(STDDEV, so, sn, nc, na)
    y.augment(so, sn)
    y.encode(0)
    y.encode(1)
    y.update(STDDEV, noise_critic=nc, noise_actor=na, keep_encoded=True)
    _assert_same_step(x, y, 'fresh with given shifts vs augment + encode + keep_encoded')


# ---------------------------------------------------------------------------------------------------- 3. nothing carries over between drivers
def test_nothing_carries_over_between_drivers():
    x, y = _pair()
    so, sn, nc, na = _draws(31)
    for e in (x, y):
        _set(e, _batch(13, B, C_, HW, A))
    x.update_phase(0, STDDEV, so, sn, nc)
    x.update_phase(1, STDDEV, noise_actor=na)
    x.update_phase(2, STDDEV)
    y.update(STDDEV, so, sn, nc, na)
    _assert_same_step(x, y, 'step 1: phases by hand vs one call')
    so, sn, nc, na = _draws(32)
    for e in (x, y):
        _set(e, _batch(14, B, C_, HW, A))
        e.augment(so, sn)
        e.update(STDDEV, noise_critic=nc, noise_actor=na, keep_augmented=True)
    _assert_same_step(x, y, 'step 2: one call on kept images')
    for e in (x, y):
        _set(e, _batch(15, B, C_, HW, A))
        e.update(STDDEV)                                    # Philox shifts and noise: the counters must have advanced alike
    _assert_same_step(x, y, 'step 3: one call, Philox')
    assert x.export_state()['steps'].tolist() == [3, 0, 3]


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_what_cannot_be_a_step_is_refused():
    from exorl_amd import _lib as L
    e = _engine(C_, HW, A, F, H, B)
    _set(e, _batch(16, B, C_, HW, A))
    e.set_train_encoder(False)
    with pytest.raises(L.ExorlError, match='kept encodings need'):          # no encodings
        e.update(STDDEV, keep_encoded=True)
    e.set_train_encoder(True)
    e.augment()
    e.encode(0)
    e.encode(1)
    with pytest.raises(L.ExorlError, match='set_train_encoder'):            # encodings, but the encoder trains
        e.update(STDDEV, keep_encoded=True)
    with pytest.raises(L.ExorlError, match='phase 3 out of range'):
        e.update_phase(3, STDDEV)


def test_a_malformed_step_struct_is_refused():
    from exorl_amd import _lib as L
    if not hasattr(L, 'PixelStep'):
        pytest.skip('exorl_pixel_step arrives with ABI 13')
    e = _engine(C_, HW, A, F, H, B)
    _set(e, _batch(17, B, C_, HW, A))
    e.augment()
    shifts = torch.zeros(B, 2, dtype=torch.int32, device=e.device)
    nxt = C.c_int32()
    for step, msg in ((L.PixelStep(STDDEV, 7, None, None, None, None), 'images=7'),
                      (L.PixelStep(STDDEV, L.PIXEL_IMAGES_AUGMENTED, shifts.data_ptr(), None, None, None), 'shifts given with images=1')):
        with pytest.raises(L.ExorlError, match=msg):
            L.check(e.lib.exorl_pixel_agent_update(e.h, C.byref(step), L.current_stream()))
        with pytest.raises(L.ExorlError, match=msg):
            L.check(e.lib.exorl_pixel_agent_update_phase(e.h, 0, C.byref(step), C.byref(nxt), L.current_stream()))
    assert e.export_state()['steps'].tolist() == [0, 0, 0]
