"""CPU checks of the sharded module step's C ABI: the library exports the phase / exchange entry points of the intrinsic-reward modules and
of the pixel engine's encoder step and RND front end, the ctypes layer declares them, and exorl_amd._lib.IntrCfg mirrors the header's
exorl_intr_cfg field for field (world_size and rank last)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ['exorl_intr_update_phase', 'exorl_intr_exchange', 'exorl_pixel_agent_encoder_step_phase', 'exorl_pixel_agent_rnd_features_phase',
       'exorl_pixel_agent_exchange']


def _header():
    return (ROOT / 'include' / 'exorl_hip.h').read_text()


def _header_intr_cfg_fields():
    body = re.search(r'typedef struct exorl_intr_cfg \{(.*?)\} exorl_intr_cfg;', _header(), re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(',')]
    return fields


def test_library_exports_the_module_dp_entry_points():
    from exorl_amd import build
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    for s in NEW:
        assert hasattr(lib, s), f'{s} is not exported by libexorl_hip.so'
    lib.exorl_abi_version.restype = ctypes.c_int
    assert lib.exorl_abi_version() == 13


def test_prototypes_declare_the_module_dp_entry_points():
    from exorl_amd import _lib
    for s in NEW:
        assert s in _lib.PROTOTYPES, s
    res, args = _lib.PROTOTYPES['exorl_intr_update_phase']
    assert res is ctypes.c_int and len(args) == 6 and args[2] is ctypes.c_int32 and args[3] is ctypes.c_int32
    assert len(_lib.PROTOTYPES['exorl_intr_exchange'][1]) == 6
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_encoder_step_phase'][1]) == 7
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_rnd_features_phase'][1]) == 8
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_exchange'][1]) == 6


def test_intr_cfg_matches_the_header():
    from exorl_amd import _lib
    ctypes_of = {'int32_t': ctypes.c_int32, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float}
    want = [(n, ctypes_of[t]) for n, t in _header_intr_cfg_fields()]
    got = [(n, t) for n, t in _lib.IntrCfg._fields_]
    assert got == want
    assert want[-2:] == [('world_size', ctypes.c_int32), ('rank', ctypes.c_int32)]


def test_exchange_constants_match_the_header():
    from exorl_amd import _lib
    h = _header()
    for name in ('INTR_XCHG_GRAD', 'INTR_XCHG_REP', 'INTR_XCHG_MOMENTS', 'XCHG_F32', 'XCHG_F64', 'XCHG_SUM', 'XCHG_GATHER'):
        assert int(re.search(rf'#define EXORL_{name}\s+(\d+)', h).group(1)) == getattr(_lib, name), name
