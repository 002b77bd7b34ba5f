"""CPU: every function include/wsscam.h declares is either swept by tests/test_gpu_scratch.py (a key of its CASES) or listed here
with the reason why it cannot read scratch.  A new entry point cannot be added without deciding which it is."""
from tests import test_gpu_scratch as sweep
from wsscam import _lib

# entry point -> why no case: it takes no workspace arena, no cached block and no staged table
NO_SCRATCH = {
    "wsc_version": "query: a constant",
    "wsc_last_error": "query: the thread's error text",
    "wsc_ctx_create": "context: creates the (empty) arena and free list",
    "wsc_ctx_destroy": "context: frees them",
    "wsc_ctx_set_option": "context: stores a path selector",
    "wsc_ctx_scratch_fill": "context: the hook itself (test_scratch_fill_argument_and_restore)",
    "wsc_ctx_scratch_fill_value": "query: the hook's current value",
    "wsc_sync": "context: stream synchronisation",
    "wsc_ctx_range_status": "query: the range flag in mapped host memory",
    "wsc_ctx_wait": "context: event record / wait",
    "wsc_ctx_mark": "context: event record",
    "wsc_ctx_wait_mark": "context: event wait on the host",
    "wsc_ctx_wait_for_mark": "context: event wait on the device",
    "wsc_device_info": "query: architecture name and CU count",
    "wsc_malloc": "memory: a caller buffer (hipMalloc)",
    "wsc_free": "memory: a caller buffer (hipFree)",
    "wsc_memcpy_h2d": "memory: copy into a caller buffer",
    "wsc_memcpy_d2h": "memory: copy out of a caller buffer",
    "wsc_memcpy_h2d_async": "memory: copy into a caller buffer",
    "wsc_memcpy_d2h_async": "memory: copy out of a caller buffer",
    "wsc_memset": "memory: memset of a caller buffer",
    "wsc_host_alloc": "memory: page-locked host memory",
    "wsc_host_free": "memory: page-locked host memory",
    "wsc_host_write_segments": "host only: writev of host segments",
    "wsc_profile_begin": "timer: event bookkeeping",
    "wsc_profile_end": "timer: event bookkeeping",
    "wsc_profile_class_name": "query: a constant string",
    "wsc_timer_begin": "timer: event record",
    "wsc_timer_end": "timer: event record and elapsed time",
    "wsc_net_destroy": "frees the net's own (hipMalloc) weights",
    "wsc_net_cam_size": "query: host-side plan of the sizes",
    "wsc_net_cam_size_hw": "query: host-side plan of the sizes",
    "wsc_net_feat_channels": "query: a field of the net",
    "wsc_net_edge_size": "query: host-side plan of the sizes",
    "wsc_net_seg_size_hw": "query: host-side plan of the sizes",
    "wsc_net_seg_tape_plan": "query: host-side plan of the tape",
    "wsc_net_trace_plan": "query: host-side plan of the ops",
    "wsc_net_set_mean_shift": "host state of the net: two floats",
    "wsc_net_get_mean_shift": "host state of the net: two floats",
    "wsc_seg_grad_destroy": "frees the object's own buffers",
    "wsc_seg_grad_layout": "query: host-side layout table",
    "wsc_irn_grad_destroy": "frees the object's own buffers",
    "wsc_irn_grad_layout": "query: host-side layout table",
    "wsc_crf_destroy": "hands the object's blocks back to the cache",
    "wsc_crf_v_destroy": "hands the object's blocks back to the cache",
    "wsc_crf_gaussian_on_chip": "query: a flag of the built lattices",
    "wsc_crf_v_num_groups": "query: a count of the built object",
}


def test_every_entry_point_is_swept_or_excused():
    declared = set(_lib.header_symbols())
    swept, excused = set(sweep.CASES), set(NO_SCRATCH)
    assert len(declared) >= 100
    assert not (swept & excused), "both swept and excused: %s" % sorted(swept & excused)
    assert not (swept - declared), "CASES names functions the header does not declare: %s" % sorted(swept - declared)
    assert not (excused - declared), "NO_SCRATCH names functions the header does not declare: %s" % sorted(excused - declared)
    missing = declared - swept - excused
    assert not missing, "neither in test_gpu_scratch.CASES nor in NO_SCRATCH: %s" % sorted(missing)
    assert all(isinstance(r, str) and r.strip() for r in NO_SCRATCH.values())


def test_every_case_id_runs():
    """CASES points at case ids the sweep really parametrises"""
    ids = set(sweep._RUNS)
    for entry, cases in sweep.CASES.items():
        assert cases and set(cases) <= ids, entry
    assert ids == {c for cases in sweep.CASES.values() for c in cases}
