"""CPU checks of the pixel step's C ABI after the step struct: exorl_amd._lib.PixelStep mirrors the header's exorl_pixel_step field for field,
one exchange query replaces the two buffer queries, the three phased calls return next_exchange, and no mode travels inside a pointer."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GONE = ['exorl_pixel_agent_grad_buffer', 'exorl_pixel_agent_bn_partials']


def _header():
    return (ROOT / 'include' / 'exorl_hip.h').read_text()


def _header_pixel_step_fields():
    body = re.search(r'typedef struct exorl_pixel_step \{(.*?)\} exorl_pixel_step;', _header(), re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.fullmatch(r'(?:const\s+)?(\w+)\s+(.*)', decl, re.S).groups()
        for n in names.split(','):
            n = n.strip()
            fields.append((n.lstrip('* '), 'pointer' if n.startswith('*') else ctype))
    return fields


def test_pixel_step_matches_the_header():
    from exorl_amd import _lib
    ctypes_of = {'int32_t': ctypes.c_int32, 'float': ctypes.c_float, 'pointer': ctypes.c_void_p}
    want = [(n, ctypes_of[t]) for n, t in _header_pixel_step_fields()]
    assert [n for n, _ in want] == ['stddev', 'images', 'shifts_obs_dev', 'shifts_next_dev', 'noise_critic_dev', 'noise_actor_dev']
    assert list(_lib.PixelStep._fields_) == want


def test_constants_match_the_header():
    from exorl_amd import _lib
    h = _header()
    for name in ('PIXEL_IMAGES_FRESH', 'PIXEL_IMAGES_AUGMENTED', 'PIXEL_IMAGES_ENCODED', 'PIXEL_XCHG_CRITIC_GRAD', 'PIXEL_XCHG_ACTOR_GRAD',
                 'PIXEL_XCHG_ENCODER_GRAD', 'PIXEL_XCHG_BN'):
        assert int(re.search(rf'#define EXORL_{name}\s+(\d+)', h).group(1)) == getattr(_lib, name), name
    assert (_lib.PIXEL_XCHG_CRITIC_GRAD, _lib.PIXEL_XCHG_ACTOR_GRAD, _lib.PIXEL_XCHG_ENCODER_GRAD, _lib.PIXEL_XCHG_BN) == (0, 1, 2, 3)


def test_library_exports_the_exchange_query_and_not_the_buffer_queries():
    from exorl_amd import _lib, build
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    assert hasattr(lib, 'exorl_pixel_agent_exchange')
    for s in GONE:
        assert not hasattr(lib, s), f'{s} is still exported by libexorl_hip.so'
        assert s not in _lib.PROTOTYPES, s
        assert f'{s}(' not in _header(), s          # the version history may still name them; no declaration does


def test_prototype_arities():
    from exorl_amd import _lib
    step = ctypes.POINTER(_lib.PixelStep)
    res, args = _lib.PROTOTYPES['exorl_pixel_agent_update']
    assert res is ctypes.c_int and len(args) == 3 and args[1] is step
    res, args = _lib.PROTOTYPES['exorl_pixel_agent_update_phase']
    assert res is ctypes.c_int and len(args) == 5 and args[2] is step and args[3] is ctypes.POINTER(ctypes.c_int32)
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_exchange'][1]) == 6
    for name, n in (('exorl_pixel_agent_encoder_step_phase', 7), ('exorl_pixel_agent_rnd_features_phase', 8)):
        args = _lib.PROTOTYPES[name][1]
        assert len(args) == n and args[-2] is ctypes.POINTER(ctypes.c_int32), name


def test_prototypes_agree_with_the_headers_parameter_counts():
    from exorl_amd import _lib
    h = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    for name in ('exorl_pixel_agent_update', 'exorl_pixel_agent_update_phase', 'exorl_pixel_agent_exchange', 'exorl_pixel_agent_encoder_step_phase',
                 'exorl_pixel_agent_rnd_features_phase'):
        params = re.search(rf'\bint {name}\((.*?)\);', h, re.S).group(1)
        assert len(params.split(',')) == len(_lib.PROTOTYPES[name][1]), name


def test_no_mode_travels_inside_a_pointer():
    assert '(const int32_t*)-' not in _header()
    for f in ('engine.py', '_lib.py'):
        assert 'c_void_p(-' not in (ROOT / 'exorl_amd' / f).read_text(), f


def test_abi_version_is_13_and_the_header_names_the_change():
    from exorl_amd import _lib
    assert _lib.load().exorl_abi_version() == 13
    version = re.search(r'#define EXORL_ABI_VERSION 13\s+/\*(.*?)\*/', _header(), re.S)
    assert version and 'exorl_pixel_step' in version.group(1).split('13:')[1]
