"""Reader of tests/golden/ingest_golden.npz (see tests/golden/make_golden_ingest.py),
shared by tests/test_ingest_cpu.py and tests/test_ingest_gpu.py."""

import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ingest_golden.npz')
FAMILIES = ('ant', 'visual', 'powder', 'one')
LOAD_KW = {'ant': {}, 'one': {}, 'visual': dict(ob_dtype=np.uint8),
           'powder': dict(ob_dtype=np.uint8, action_dtype=np.int32)}
_cache = {}


def golden():
    """Every array of the fixture (read once; treat as read-only)."""
    if not _cache:
        with np.load(PATH, allow_pickle=False) as f:
            for k in f.files:
                v = f[k]
                v.setflags(write=False)
                _cache[k] = v
    return _cache


def raw_columns(g, family):
    p = f'raw_{family}_'
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p)}


def expected_load(g, family, mode, info):
    """The reference's load of one family, rebuilt from the fixture: key order,
    dtypes and shapes from the key strings, values from exp_* or the raw column."""
    out = {}
    for s in g[f'keys_{family}_{mode}_{"info" if info else "noinfo"}']:
        k, dtype, shape = str(s).split('|')
        shape = tuple(int(v) for v in shape.split(',') if v)
        name = f'exp_{family}_{mode}_{k}'
        v = g[name] if name in g else g[f'raw_{family}_{k}']
        assert v.dtype.name == dtype and v.shape == shape, (family, mode, k)
        out[k] = v
    return out
