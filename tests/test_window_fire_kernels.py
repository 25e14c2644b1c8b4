"""The window firing kernels, called directly, against the plain model (needs an MI355X).

tests/window_model.py states what window_fire_kernel, window_fire_multi_kernel<1> / <4>,
window_refire_multi_kernel, fire_pack_kernel, dirty_clear_kernel, scatter_partials_kernel,
step_begin_kernel / step_finish_kernel, keygroup_kernel and table_insert_kernel compute;
test_window_model.py checks that model against the C++ twin on the same inputs. Here the inputs
of tests/window_cases.py go to the HIP kernels: window_fire_many and gpu_window_refire_many
through the native module, everything else through the mxstream.ops.kernels wrappers.

Each case is one small launch at a shape chosen for what can go wrong there: pane counts around
kFireP (8) and up to the whole ring, windows that wrap the ring or start at a negative pane,
tables of 1 / 1023 / 4096 / 4097 slots (one workgroup round of window_fire is 4096), slot lists
shorter than their buffer, out_cap below the row count, 33 windows (a second pack), the U = 4
variant from 65,536 slots on, second grid-stride rounds, staging regions that overflow, dirty
masks, the LDS-stack epilogue next to the register chain, every aggregate with wrapping sums,
signed zeros, infinities, subnormals and NaNs. The GPU's row order is unspecified, so rows are
compared sorted by their (unique) key; every comparison is bit for bit, and every output and
staging word the kernel had no reason to write must still hold its sentinel.
"""
import pytest
import torch

import window_cases as C
import window_model as M

pytestmark = pytest.mark.gpu


# ---- window_fire_kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("nslots,p0,npanes,only_dirty", C.GEOM, ids=C.ids(C.GEOM))
def test_fire_geometry(gpu_device, native, nslots, p0, npanes, only_dirty):
    C.case_geometry(gpu_device, False, nslots, p0, npanes, only_dirty)


@pytest.mark.parametrize("agg", M.AGGS)
def test_fire_aggregate(gpu_device, native, agg):
    C.case_aggregate(gpu_device, False, agg)


@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_fire_epilogue(gpu_device, native, name):
    C.case_epilogue(gpu_device, False, name)


@pytest.mark.parametrize("name", C.OUTPUTS)
def test_fire_outputs(gpu_device, native, name):
    C.case_outputs(gpu_device, False, name)


@pytest.mark.parametrize("list_n,only_dirty", C.LIST, ids=C.ids(C.LIST))
def test_fire_slot_list(gpu_device, native, list_n, only_dirty):
    C.case_list(gpu_device, False, list_n, only_dirty)


def test_fire_second_round(gpu_device, native):
    """1024 * 4096 + 4097 slots: workgroups 0 and 1 run a second, partial round."""
    C.case_second_round(gpu_device, False)


# ---- window_fire_multi_kernel + fire_pack_kernel ------------------------------------------------
@pytest.mark.parametrize("nslots,k,key32", C.MANY_SMALL, ids=C.ids(C.MANY_SMALL))
def test_fire_many_small(gpu_device, native, nslots, k, key32):
    C.case_many_small(gpu_device, False, nslots, k, key32)


@pytest.mark.parametrize("nslots", C.MANY_BIG)
def test_fire_many_big(gpu_device, native, nslots):
    C.case_many_big(gpu_device, False, nslots)


def test_fire_many_region_below_table_raises(gpu_device, native):
    st = C.build_state(17, 255, 64, empty_panes=C.MANY_EMPTY)
    with pytest.raises(ValueError, match="staging region"):
        C.check_fire_many(gpu_device, st, False, agg=M.AGG_SUM_I64, wins=C.many_wins(2),
                          key32=False, region=st.nslots - 1)


# ---- window_refire_multi_kernel + fire_pack_kernel ----------------------------------------------
@pytest.mark.parametrize("list_n,k,variant", C.REFIRE, ids=C.ids(C.REFIRE))
def test_refire(gpu_device, native, list_n, k, variant):
    C.case_refire(gpu_device, list_n, k, variant)


@pytest.mark.parametrize("variant", list(C.REFIRE_VARIANTS))
def test_refire_small_region(gpu_device, native, variant):
    """The first window has more rows than a region holds: the flag, `region` of its rows, the
    later windows intact."""
    C.case_refire_small_region(gpu_device, variant)


@pytest.mark.parametrize("name", C.REFIRE_FALSE)
def test_refire_cannot_fuse(gpu_device, native, name):
    C.case_refire_false(gpu_device, name)


# ---- the small kernels of the path --------------------------------------------------------------
@pytest.mark.parametrize("list_n,p_lo,np_,delta", C.DIRTY_CLEAR, ids=C.ids(C.DIRTY_CLEAR))
def test_dirty_clear(gpu_device, native, list_n, p_lo, np_, delta):
    C.check_dirty_clear(gpu_device, list_n, p_lo, np_, delta)


@pytest.mark.parametrize("n_dev,geom,max_par,hash_mode", C.SCATTER, ids=C.ids(C.SCATTER))
def test_scatter_partials(gpu_device, native, n_dev, geom, max_par, hash_mode):
    C.check_scatter(gpu_device, False, n_dev, geom, max_par, hash_mode)


def test_scatter_partials_hot_bucket(gpu_device, native):
    C.check_scatter_hot(gpu_device, False)


@pytest.mark.parametrize("nb", [1, 255, 16384])
def test_step_begin(gpu_device, native, nb):
    C.check_step_begin(gpu_device, nb)


@pytest.mark.parametrize("flags,event_mode,lm,ovf", C.STEP_FINISH, ids=C.ids(C.STEP_FINISH))
def test_step_finish(gpu_device, native, flags, event_mode, lm, ovf):
    C.check_step_finish(gpu_device, flags, event_mode, lm, ovf)


@pytest.mark.parametrize("hash_mode,max_par", C.KEYGROUPS, ids=C.ids(C.KEYGROUPS))
def test_keygroups(gpu_device, native, hash_mode, max_par):
    C.check_keygroups(gpu_device, hash_mode, max_par)


@pytest.mark.parametrize("nsub_log2,cap_log2", C.TABLE, ids=C.ids(C.TABLE))
def test_table_insert(gpu_device, native, nsub_log2, cap_log2):
    C.check_table_insert(gpu_device, nsub_log2, cap_log2)
