"""The graph record's layout (``dr_graph_records``) against the LDS carves that
stage it with one linear copy (host side, no GPU).

A record is the Z-input carve's input regions as they lie in LDS, so one copy
of ``dr_graph_record_words`` words starting at the carve's ``z`` must put every
region where the kernel reads it: the record's section offsets
(``dr_debug_graph_record``) equal the offsets of ``dr_debug_carve_ginet_z`` and
of ``dr_debug_carve_ginet_acc`` (both parities of the prefetch layout) relative
to ``z``, for every graph and stride of ``test_lds_carves``.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
from test_lds_carves import GINET_GRAPHS, _carve, r4

from deeprank2_amd import _lib
from deeprank2_amd.store import REC_DESC_DTYPE, record_words

SECTIONS = ("z", "cl0", "p1rp", "p1c", "p1trp", "p1tc", "m1p", "m1i")
F_ZS = [(F, KP + d) for F, KP in ((1, 32), (30, 32), (32, 32), (33, 64), (50, 64)) for d in (0, 2, 4)]


def _record(N, K0, P1, K1, alias, zs):
    offs = (ctypes.c_int32 * 9)()
    assert _lib.load().dr_debug_graph_record((ctypes.c_int32 * 6)(N, K0, P1, K1, alias, zs), offs) == 0
    return dict(zip((*SECTIONS, "total"), offs))


def _padded_sum(N, K0, P1, K1, alias, zs):
    pooled = r4(K0 + 1) + r4(P1)
    return r4(N * zs) + r4(N) + pooled * (1 if alias else 2) + r4(K1 + 1) + r4(K0)


@pytest.mark.parametrize(("N", "E", "K0", "P1", "K1", "alias", "OUT"), GINET_GRAPHS)
@pytest.mark.parametrize(("F", "zs"), F_ZS)
def test_record_sections_are_the_z_carve_offsets_from_z(N, E, F, K0, P1, K1, alias, OUT, zs):
    rec = _record(N, K0, P1, K1, alias, zs)
    carve = _carve("ginet_z", [N, E, F, K0, P1, K1, alias, OUT, zs])
    assert carve["z"] % 4 == 0
    for k in SECTIONS:
        assert carve[k] - carve["z"] == rec[k], (k, carve[k], carve["z"], rec[k])
    assert rec["z"] == 0 and rec["total"] % 4 == 0
    if alias:
        assert (rec["p1trp"], rec["p1tc"]) == (rec["p1rp"], rec["p1c"])
    # the copy ends inside the carve, and on the first region that is not an input
    assert carve["z"] + rec["total"] == carve["key"] <= carve["total"]


@pytest.mark.parametrize(("N", "E", "K0", "P1", "K1", "alias", "OUT"), GINET_GRAPHS)
@pytest.mark.parametrize(("F", "zs"), F_ZS)
@pytest.mark.parametrize("par", [0, 1])
def test_record_sections_are_the_prefetch_layout_offsets_from_z(N, E, F, K0, P1, K1, alias, OUT, zs, par):
    """The graph is smaller than the batch maxima in every size: its record is
    packed from the start of its parity segment and ends inside it."""
    maxima = [N + 7, E + 50, K0 + 2, P1 + 5, K1 + 1]
    rec = _record(N, K0, P1, K1, alias, zs)
    carve = _carve("ginet_acc", [N, E, F, K0, P1, K1, alias, OUT, *maxima, par, zs])
    seg = carve["$in1"] if par else carve["$in0"]
    assert carve["z"] == seg
    for k in SECTIONS:
        assert carve[k] - carve["z"] == rec[k], (k, par)
    assert seg + rec["total"] <= seg + (carve["$in1"] - carve["$in0"])
    assert _record(*maxima[:1], *maxima[2:], alias, zs)["total"] == carve["$in1"] - carve["$in0"]  # the segment: the maxima's record


@pytest.mark.parametrize(("N", "E", "K0", "P1", "K1", "alias", "OUT"), GINET_GRAPHS)
@pytest.mark.parametrize("zs", [32, 34, 36, 64, 68])
def test_record_words_is_the_sum_of_the_padded_regions(N, E, K0, P1, K1, alias, OUT, zs):
    want = _padded_sum(N, K0, P1, K1, alias, zs)
    assert _lib.load().dr_graph_record_words(N, K0, P1, K1, alias, zs) == want == _record(N, K0, P1, K1, alias, zs)["total"]
    assert int(record_words(N, K0, P1, K1, alias, zs)) == want  # the store's host mirror
    v = record_words(np.array([N, 1]), np.array([K0, 1]), np.array([P1, 0]), np.array([K1, 1]), alias, zs)
    assert v.tolist() == [want, _padded_sum(1, 1, 0, 1, alias, zs)]


def test_record_descriptor_has_the_sizes_where_the_graph_descriptor_has_them():
    from deeprank2_amd.store import DESC_DTYPE  # noqa: PLC0415

    assert REC_DESC_DTYPE.itemsize == DESC_DTYPE.itemsize == 64  # noqa: PLR2004
    assert REC_DESC_DTYPE.fields["rec0"][1] == DESC_DTYPE.fields["node0"][1] == 0
    for k in ("n_nodes", "n_edges", "n_k0", "n_p1", "n_k1", "gid"):
        assert REC_DESC_DTYPE.fields[k][1] == DESC_DTYPE.fields[k][1], k


def test_new_entries_check_their_arguments():
    """Every refusal below is decided on the host, before any launch."""
    lib = _lib.load()
    E_ARG = -1  # DR_E_ARG
    st = _lib.GraphStoreC()
    st.n_graphs, st.n_feat = 4, 30
    w, p = _lib.GinetWeightsC(), _lib.PassC()
    ok = 4096  # (a 16-byte aligned non-null address: never dereferenced by a refused call)
    assert lib.dr_graph_record_words(-1, 1, 0, 1, 1, 36) == -1
    assert lib.dr_graph_record_words(1, 1, 0, 1, 1, 0) == -1
    assert lib.dr_debug_graph_record(None, None) == E_ARG
    # dr_graph_records: null pointers, a stride below F, a range outside the store, a misaligned buffer
    assert lib.dr_graph_records(None, ok, 36, ok, 0, 1, None) == E_ARG
    assert lib.dr_graph_records(st, None, 36, ok, 0, 1, None) == E_ARG
    assert lib.dr_graph_records(st, ok, 36, None, 0, 1, None) == E_ARG
    assert lib.dr_graph_records(st, ok, 29, ok, 0, 1, None) == E_ARG
    assert lib.dr_graph_records(st, ok, 36, ok, 3, 2, None) == E_ARG
    assert lib.dr_graph_records(st, ok, 36, ok, -1, 1, None) == E_ARG
    assert lib.dr_graph_records(st, ok + 4, 36, ok, 0, 1, None) == E_ARG
    # the record passes: no records, no descriptors, a misaligned buffer, a stride below K or odd
    assert lib.dr_ginet_graph_pass_rec(st, ok, 1, w, p, 1024, None, 36, None) == E_ARG
    assert lib.dr_ginet_graph_pass_rec(st, None, 1, w, p, 1024, ok, 36, None) == E_ARG
    assert lib.dr_ginet_graph_pass_rec(st, ok, 1, w, p, 1024, ok + 8, 36, None) == E_ARG
    assert lib.dr_ginet_graph_pass_rec(st, ok, 1, w, p, 1024, ok, 30, None) == E_ARG
    assert lib.dr_ginet_graph_pass_rec(st, ok, 1, w, p, 1024, ok, 35, None) == E_ARG
    assert lib.dr_ginet_graph_pass_rec(None, ok, 1, w, p, 1024, ok, 36, None) == E_ARG
    assert lib.dr_ginet_acc_pass_rec(st, ok, ok, 1, w, p, 1024, 1024, 1, None, None, None, 36, None) == E_ARG
    assert lib.dr_ginet_acc_pass_rec(st, ok, None, 1, w, p, 1024, 1024, 1, None, None, ok, 36, None) == E_ARG
    assert lib.dr_ginet_acc_pass_rec(st, ok, ok, 1, w, p, 1024, -1, 1, None, None, ok, 36, None) == E_ARG
    assert lib.dr_ginet_acc_pass_rec(st, ok, ok, 1, w, p, 1024, 1024, 1, None, None, ok, 30, None) == E_ARG
