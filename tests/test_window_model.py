"""tests/window_model.py against the C++ twin (csrc/kernels_cpu.cpp), on the CPU.

The model states what the window firing kernels compute; here every case list of
tests/window_cases.py -- the same inputs test_window_fire_kernels.py gives the HIP kernels --
goes through the twin: window_fire and window_fire_many(cuda=False), dirty_clear,
scatter_partials, step_begin / step_finish, keygroups and table_insert on CPU tensors. The twin
visits slots in order, so rows are compared in order. The fused re-firing has no twin: the model
of it is checked against the per-window model, and its "cannot be fused" answers by construction.
"""
import numpy as np
import pytest
import torch

import window_cases as C
import window_model as M

CPU = torch.device("cpu")


# ---- the model's own pieces ---------------------------------------------------------------------
@pytest.mark.parametrize("agg", M.AGGS)
def test_identity_is_neutral(agg):
    st = C.build_state(3, 257, 4, agg=agg)
    a = st.acc[np.flatnonzero(~np.isnan(st.acc.view(np.float64)))] if agg in C.F64_AGGS else st.acc
    ident = np.full(len(a), M.identity(agg), np.uint64)
    got = M.combine(agg, ident, a)
    if agg in (M.AGG_SUM_F64, M.AGG_AVG_F64):       # 0.0 + -0.0 is 0.0: equal as values
        assert np.array_equal(got.view(np.float64), a.view(np.float64))
    else:
        assert np.array_equal(got, a)


def test_combine_edges():
    u = lambda x: np.array([x & M.U64], dtype=np.uint64)
    f = lambda x: np.array([x], dtype=np.float64).view(np.uint64)
    assert M.combine(M.AGG_SUM_I64, u(M.I64_MAX), u(1))[0] == 1 << 63            # wraps
    assert M.combine(M.AGG_MIN_I64, u(M.I64_MIN), u(5))[0] == 1 << 63
    assert M.combine(M.AGG_SUM_F64, f(1e16), f(1.0))[0] == f(1e16)[0]            # one rounding
    nan = u(C.NANS[0])
    assert M.combine(M.AGG_MIN_F64, nan, f(2.0))[0] == f(2.0)[0]                 # (nan < b) ? a : b
    assert M.combine(M.AGG_MIN_F64, f(2.0), nan)[0] == nan[0]
    assert M.combine(M.AGG_MAX_F64, f(0.0), f(-0.0))[0] == f(-0.0)[0]            # (0 > -0) ? a : b
    assert M.result(M.AGG_AVG_I64, u(7), np.uint32(2)) == 3.5
    assert M.result(M.AGG_COUNT, u(99), np.uint32(4)) == 4.0
    assert M.result(M.AGG_SUM_I64, u(-3), np.uint32(1)) == -3.0


def test_keygroups_scalar_and_vectorised_agree():
    from mxstream.utils import hashing as H

    keys = np.random.default_rng(1).integers(0, 1 << 64, 5000, dtype=np.uint64)
    jh = ((keys ^ (keys >> np.uint64(32))) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for mp in (128, 120):
        assert np.array_equal(M.keygroups(keys, mp), H.key_groups_of_java_hashes(jh, mp))


@pytest.mark.parametrize("k", [1, 4, 32])
@pytest.mark.parametrize("clear", [False, True])
def test_refire_model_equals_per_window_fire(k, clear):
    st, slots = C.refire_input()
    mp, fp, _ = C.programs("both-chain")
    wins = C.refire_wins(k)
    got = M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots[:3000], 0, 0, clear=clear)
    lo = 0
    for (p0, n, ws, we), hi in zip(wins, got[1].tolist()):
        want = M.fire(st, M.AGG_SUM_I64, p0, n, True, ws, we, mp, fp, slots[:3000])
        C.assert_rows(got[0][lo:hi], want, True)
        lo = hi
    assert lo == len(got[0]) > 0
    if clear:
        after = got[2]
        listed = np.zeros(st.nslots, bool)
        listed[slots[:3000]] = True
        assert not after.mark[listed].any()
        assert np.array_equal(after.mark[~listed], st.mark[~listed])
        d0, d1 = st.dirty.reshape(16, -1), after.dirty.reshape(16, -1)
        c0 = st.cnt.reshape(16, -1)
        assert np.array_equal(d1[:, ~listed], d0[:, ~listed])
        # the union is the whole ring: a listed slot keeps exactly its dirty bytes without a count
        assert np.array_equal(d1[:, listed], d0[:, listed] * (c0[:, listed] == 0))


def test_refire_model_mask_drops_rows():
    st, slots = C.refire_input()
    dlo, dmask, epi, _, _ = C.REFIRE_VARIANTS["mask31-chain-k32-clear"]
    mp, fp, _ = C.programs(epi)
    wins = C.refire_wins(4)
    every = M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots, 0, 0)
    some = M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots, dlo, dmask, clear=True)
    assert (some[1] < every[1]).all()
    # pane 21 is bit 31 of the mask, which stands for no pane: its dirty bytes stay
    after, gi = some[2], st.index(21, slots)
    assert np.array_equal(after.dirty[gi], st.dirty[gi]) and st.dirty[gi].any()
    gi = st.index(20, slots)
    assert not (after.dirty[gi] & (st.cnt[gi] != 0)).any()


@pytest.mark.parametrize("name", C.REFIRE_FALSE)
def test_refire_model_cannot_fuse(name):
    st, wins, has_list = C.refire_false_input(name)
    mp, fp, _ = C.programs("both-chain")
    slots = C.refire_input()[1] if has_list else None
    assert M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots) is None
    if name == "union17":       # one pane less and it fuses
        wins[1] = (18, 8) + wins[1][2:]
        assert M.refire_many(st, M.AGG_SUM_I64, mp, fp, wins, slots) is not None


def test_refire_small_region_inputs():
    st, slots = C.refire_input()
    for variant in C.REFIRE_VARIANTS:
        C.refire_small_region(st, slots, variant)


# ---- the twin against the model, on every case list ---------------------------------------------
@pytest.mark.parametrize("nslots,p0,npanes,only_dirty", C.GEOM, ids=C.ids(C.GEOM))
def test_fire_geometry(nslots, p0, npanes, only_dirty):
    C.case_geometry(CPU, True, nslots, p0, npanes, only_dirty)


@pytest.mark.parametrize("agg", M.AGGS)
def test_fire_aggregate(agg):
    C.case_aggregate(CPU, True, agg)


@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_fire_epilogue(name):
    C.case_epilogue(CPU, True, name)


@pytest.mark.parametrize("name", C.OUTPUTS)
def test_fire_outputs(name):
    C.case_outputs(CPU, True, name)


@pytest.mark.parametrize("list_n,only_dirty", C.LIST, ids=C.ids(C.LIST))
def test_fire_slot_list(list_n, only_dirty):
    C.case_list(CPU, True, list_n, only_dirty)


def test_fire_second_round():
    C.case_second_round(CPU, True)


@pytest.mark.parametrize("nslots,k,key32", C.MANY_SMALL, ids=C.ids(C.MANY_SMALL))
def test_fire_many_small(nslots, k, key32):
    C.case_many_small(CPU, True, nslots, k, key32)


@pytest.mark.parametrize("nslots", C.MANY_BIG)
def test_fire_many_big(nslots):
    C.case_many_big(CPU, True, nslots)


@pytest.mark.parametrize("list_n,p_lo,np_,delta", C.DIRTY_CLEAR, ids=C.ids(C.DIRTY_CLEAR))
def test_dirty_clear(list_n, p_lo, np_, delta):
    C.check_dirty_clear(CPU, list_n, p_lo, np_, delta)


@pytest.mark.parametrize("n_dev,geom,max_par,hash_mode", C.SCATTER, ids=C.ids(C.SCATTER))
def test_scatter_partials(n_dev, geom, max_par, hash_mode):
    C.check_scatter(CPU, True, n_dev, geom, max_par, hash_mode)


def test_scatter_partials_hot_bucket():
    C.check_scatter_hot(CPU, True)


@pytest.mark.parametrize("nb", [1, 255, 16384])
def test_step_begin(nb):
    C.check_step_begin(CPU, nb)


@pytest.mark.parametrize("flags,event_mode,lm,ovf", C.STEP_FINISH, ids=C.ids(C.STEP_FINISH))
def test_step_finish(flags, event_mode, lm, ovf):
    C.check_step_finish(CPU, flags, event_mode, lm, ovf)


@pytest.mark.parametrize("hash_mode,max_par", C.KEYGROUPS, ids=C.ids(C.KEYGROUPS))
def test_keygroups(hash_mode, max_par):
    C.check_keygroups(CPU, hash_mode, max_par)


@pytest.mark.parametrize("nsub_log2,cap_log2", C.TABLE, ids=C.ids(C.TABLE))
def test_table_insert(nsub_log2, cap_log2):
    C.check_table_insert(CPU, nsub_log2, cap_log2)
