"""Host side of the 20 cross-entropy entry points (plain, _w, _f, _s of dsrl_ce_fwd / dsrl_ce_bwd / dsrl_ce_fused / dsrl_convt2x2_fwd_ce /
dsrl_convt2x2_bwd_ce): every one of them returns its argument errors before any HIP call, so what they refuse and in which words is pinned
here without a GPU; and the one helper of functional.py that names the entry point of a (weights, gamma, eps) triple."""
import math

import pytest

from dualsuperreslearningforsemseg_amd import _lib
from dualsuperreslearningforsemseg_amd import functional as HF

BADARG = -1                                         # include/dsrl_hip.h: DSRL_E_BADARG
FAMILIES = ['dsrl_ce_fwd', 'dsrl_ce_bwd', 'dsrl_ce_fused', 'dsrl_convt2x2_fwd_ce', 'dsrl_convt2x2_bwd_ce']
SUFFIXES = ['', '_w', '_f', '_s']
ENTRIES = [f + s for f in FAMILIES for s in SUFFIXES]
BAD_GAMMA = [-1.0, float('nan'), float('inf')]
BAD_EPS = [-1e-30, 1.0000001, float('nan')]


def _null_call(name, scalar=None):
    """The entry point with every pointer null and every integer 0; its one float (gamma or eps) = `scalar`.  -> (code, message)."""
    lib = _lib.load()
    args = [None if t is _lib.fp else (scalar if t is _lib.f32 else 0) for t in _lib.PROTOTYPES[name][1]]
    assert (scalar is not None) == (_lib.f32 in _lib.PROTOTYPES[name][1])
    code = getattr(lib, name)(*args)
    return code, lib.dsrl_last_error().decode()


def _as_c_prints(v):
    """printf('%g') of the float the library received."""
    return 'nan' if math.isnan(v) else ('inf' if math.isinf(v) else '%g' % _lib.f32(v).value)


def test_the_table_has_the_twenty():
    assert len(ENTRIES) == 20 and all(n in _lib.PROTOTYPES for n in ENTRIES)


@pytest.mark.parametrize('name', ENTRIES)
def test_a_null_first_pointer_is_a_bad_argument_in_the_entrys_own_name(name):
    code, msg = _null_call(name, 2.0 if name.endswith('_f') else (0.1 if name.endswith('_s') else None))
    assert code == BADARG
    assert msg.startswith(name[len('dsrl_'):] + ': bad arguments'), msg


@pytest.mark.parametrize('gamma', BAD_GAMMA)
@pytest.mark.parametrize('name', [f + '_f' for f in FAMILIES])
def test_a_bad_gamma_is_refused_first(name, gamma):
    code, msg = _null_call(name, gamma)
    assert code == BADARG
    assert msg == f'{name[len("dsrl_"):]}: gamma = {_as_c_prints(gamma)} is not a finite number >= 0', msg


@pytest.mark.parametrize('eps', BAD_EPS)
@pytest.mark.parametrize('name', [f + '_s' for f in FAMILIES])
def test_a_bad_eps_is_refused_first(name, eps):
    code, msg = _null_call(name, eps)
    assert code == BADARG
    assert msg == f'{name[len("dsrl_"):]}: eps = {_as_c_prints(eps)} is not a number in [0, 1]', msg


@pytest.mark.parametrize('name', [f + s for f in FAMILIES for s in ('_f', '_s')])
def test_gamma_or_eps_of_zero_reports_as_the_weighted_sibling(name):
    sib = name[:-2] + '_w'
    assert _null_call(name, 0.0) == _null_call(sib)
    assert _null_call(name, -0.0) == _null_call(sib)
    assert _null_call(sib)[1].startswith(sib[len('dsrl_'):] + ': bad arguments')


# ---- functional._ce_variant: (class-weight table, gamma, eps) -> (suffix of the entry point, what follows ignore_index in its arguments)
class _Table:                                       # stands in for a class_weight_table: the helper only asks for its pointer
    def data_ptr(self):
        return 0x1000


KINDS = {'': (None, 0.0, 0.0), '_w': (_Table(), 0.0, 0.0), '_f': (_Table(), 2.0, 0.0), '_s': (_Table(), 0.0, 0.1)}
# the workspace query each call site in functional.py makes before its call (dsrl_ce_bwd and dsrl_convt2x2_bwd_ce have none of their own)
QUERIES = {'dsrl_ce_fwd': 'dsrl_ce%s_workspace_bytes', 'dsrl_ce_fused': 'dsrl_ce_fused%s_workspace_bytes',
           'dsrl_convt2x2_fwd_ce': 'dsrl_convt2x2_fwd_ce%s_workspace_bytes'}
AFTER_IGNORE_INDEX = {'dsrl_ce_fwd': 6, 'dsrl_ce_bwd': 6, 'dsrl_ce_fused': 6, 'dsrl_convt2x2_fwd_ce': 11, 'dsrl_convt2x2_bwd_ce': 5}


def test_the_helper_keeps_the_order_of_the_ladders_it_replaces():
    t = _Table()
    assert HF._ce_variant(None, 0.0, 0.0) == ('', ())
    assert HF._ce_variant(t, 0.0, 0.0) == ('_w', (0x1000,))
    assert HF._ce_variant(t, 2.0, 0.0) == ('_f', (0x1000, 2.0))
    assert HF._ce_variant(t, 0.0, 0.25) == ('_s', (0x1000, 0.25))


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('kind', SUFFIXES)
def test_the_helper_names_a_registered_entry_of_the_arity_the_call_site_passes(family, kind):
    sfx, extra = HF._ce_variant(*KINDS[kind])
    assert sfx == kind
    plain = _lib.PROTOTYPES[family][1]
    args = _lib.PROTOTYPES[family + sfx][1]             # KeyError: the helper named an entry point that is not registered
    assert len(args) == len(plain) + len(extra)         # the call site passes the plain arguments with `extra` after ignore_index
    k = AFTER_IGNORE_INDEX[family]
    assert args[:k] + args[k + len(extra):] == plain    # ... and that is where the variant's prototype has its own
    assert args[k:k + len(extra)] == [_lib.fp, _lib.f32][:len(extra)]
    if family in QUERIES:
        assert _lib.PROTOTYPES[QUERIES[family] % sfx][1] == _lib.PROTOTYPES[QUERIES[family] % ''][1]
