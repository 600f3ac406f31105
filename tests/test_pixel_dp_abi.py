"""CPU checks of the data-parallel pixel step's C ABI: the library exports the phase / exchange / communicator entry points, the ctypes
layer declares them, and exorl_amd._lib.PixelCfg mirrors the header's exorl_pixel_cfg field for field (world_size last)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ['exorl_pixel_agent_update_phase', 'exorl_pixel_agent_exchange', 'exorl_pixel_agent_set_comm']


def _header_pixel_cfg_fields():
    txt = (ROOT / 'include' / 'exorl_hip.h').read_text()
    body = re.search(r'typedef struct exorl_pixel_cfg \{(.*?)\} exorl_pixel_cfg;', txt, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(',')]
    return fields


def test_library_exports_the_pixel_dp_entry_points():
    from exorl_amd import build
    lib = ctypes.CDLL(str(build.build(force=False, verbose=False)))
    for s in NEW:
        assert hasattr(lib, s), f'{s} is not exported by libexorl_hip.so'


def test_prototypes_declare_the_pixel_dp_entry_points():
    from exorl_amd import _lib
    for s in NEW:
        assert s in _lib.PROTOTYPES, s
    res, args = _lib.PROTOTYPES['exorl_pixel_agent_update_phase']
    assert res is ctypes.c_int and len(args) == 5 and args[1] is ctypes.c_int32 and args[2] is ctypes.POINTER(_lib.PixelStep)
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_exchange'][1]) == 6
    assert len(_lib.PROTOTYPES['exorl_pixel_agent_set_comm'][1]) == 2


def test_pixel_cfg_matches_the_header():
    from exorl_amd import _lib
    ctypes_of = {'int32_t': ctypes.c_int32, 'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float}
    want = [(n, ctypes_of[t]) for n, t in _header_pixel_cfg_fields()]
    got = [(n, t) for n, t in _lib.PixelCfg._fields_]
    assert got == want
    assert want[-1] == ('world_size', ctypes.c_int32)
