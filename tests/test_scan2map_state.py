"""Host state of the batched scan-to-map context (the per-map and snapshot records of vilf_s2m.hip): snapshot / rewind through both of its routes — the live
snapshot that is swapped back and the saved copy — for ordered maps and for maps as initialised, the rule that an upload outside a step drops the snapshot, and
re-creating a batch on a solver. Everything is compared bit for bit: a step replayed from a snapshot has to equal the step first taken from it, for two streams
with different maps, so that a mix-up between streams or between the two local maps shows."""
import numpy as np
import pytest
from s2m_scene import scene, scans as make_scans

CAPS = (512, 512, 16384, 16384)


@pytest.fixture(scope="module")
def room():
    me, ms = scene(2)
    return me, ms, make_scans(me, ms, 4)


def _batch(opts, room, n_streams=2, solver=None):
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    me, ms, _ = room
    s = solver or BackendSolver(opts); b = Scan2MapBatch(s, n_streams, *CAPS)
    for i in range(n_streams):
        b.localMapInited(i, me[::i + 1], ms[::i + 1])            # every stream its own map
    return s, b


def _set_scan(b, scan):
    for i in range(b.n):
        b.set_scan(i, scan[0][:150 - 45 * i], scan[1][:400 - 100 * i])


def _results(b):
    return [bytes(r) for r in b.results()]


def _maps(b):
    return [b.getMapCloud(i, w).tobytes() for i in range(b.n) for w in (0, 1)]


def _step(b, scan):
    _set_scan(b, scan); b.step()
    return _results(b), _maps(b)


def _no_snapshot(b):
    from vil_fusion_amd.lib import VilfError
    with pytest.raises(VilfError, match=r"status -1: .*no snapshot"):        # VILF_ERR_INVALID_ARGUMENT
        b.rewind()


@pytest.mark.gpu
def test_saved_snapshot_rewind_equals_a_replay(opts, room):
    """the snapshot is copied aside because two steps run after it; a step replayed from that copy equals the step first taken from the snapshot, twice over"""
    scan = room[2]
    s, b = _batch(opts, room)
    _step(b, scan[0]); _step(b, scan[1])                             # ordered maps
    _set_scan(b, scan[2]); b.snapshot()
    first = _step(b, scan[2])
    assert first[0][0] != first[0][1] and first[1][0] != first[1][2], "the two streams differ"
    _step(b, scan[3])                                                # overwrites the buffers the snapshot lived in: it is saved first
    for _ in range(2):
        b.rewind()
        assert _step(b, scan[2]) == first
    s.close()


@pytest.mark.gpu
def test_live_rewind_repeated(opts, room):
    """snapshot, step, rewind, rewind (the buffers are already swapped back), step: the first step again; a rewind with no step in between changes nothing"""
    scan = room[2]
    s, b = _batch(opts, room)
    _step(b, scan[0]); _step(b, scan[1])
    before = _maps(b)
    _set_scan(b, scan[2]); b.snapshot()
    b.rewind()
    assert _maps(b) == before
    first = _step(b, scan[2])
    assert first[1] != before
    b.rewind(); b.rewind()
    assert _maps(b) == before
    b.step()                                                         # (the scan is still resident)
    assert (_results(b), _maps(b)) == first
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grid_first", [False, True])
def test_snapshot_of_maps_as_initialised(opts, room, grid_first):
    """A snapshot of maps no step has ordered yet: the rewind restores the order state and the per-stream length of the cell-major prefix, not only the points —
    a raw cloud comes back from getMapCloud as given, byte for byte, and the step after the rewind equals the first. grid_first: stream 0 is initialised from a
    downloaded voxel grid (stored in cell-major order, handed out in PCL order), stream 1 from a raw cloud: the two prefix lengths differ."""
    from vil_fusion_amd.estimator import BackendSolver, Scan2MapBatch
    me, ms, scan = room
    given = [(me, ms), (me[::2], ms[::2])]
    if grid_first:
        s0, b0 = _batch(opts, room, 1)
        _step(b0, scan[0])
        given[0] = (b0.getMapCloud(0, 0).copy(), b0.getMapCloud(0, 1).copy())
        s0.close()
    s = BackendSolver(opts); b = Scan2MapBatch(s, 2, *CAPS)
    for i in (0, 1):
        b.localMapInited(i, *given[i])
    as_given = [given[i][w].tobytes() for i in (0, 1) for w in (0, 1)]
    assert _maps(b) == as_given
    _set_scan(b, scan[1]); b.snapshot()
    assert _maps(b) == as_given
    first = _step(b, scan[1])
    b.rewind()
    assert _maps(b) == as_given
    b.step()
    assert (_results(b), _maps(b)) == first
    _step(b, scan[2])                                                # and through the saved copy
    b.rewind()
    assert _maps(b) == as_given
    assert _step(b, scan[1]) == first
    s.close()


@pytest.mark.gpu
def test_an_upload_outside_a_step_drops_the_snapshot(opts, room):
    """localMapInited and copy_stream write a stream's map where a live snapshot sits: the snapshot is dropped and rewind reports that there is none, instead of
    restoring the order and counts of contents that are gone. A fresh snapshot afterwards holds the new contents."""
    me, ms, scan = room
    s, b = _batch(opts, room)
    _no_snapshot(b)                                                  # none taken yet
    _step(b, scan[0])
    for write in (lambda: b.localMapInited(1, me[::3], ms[::3]), lambda: b.copy_stream(0, 1)):
        b.snapshot()
        write()
        _no_snapshot(b)
        now = _maps(b)
        _set_scan(b, scan[1]); b.snapshot()
        first = _step(b, scan[1])
        b.rewind()
        assert _maps(b) == now
        b.step()
        assert (_results(b), _maps(b)) == first
    assert now[:2] == now[2:], "after copy_stream stream 1 holds stream 0's maps"
    s.close()


@pytest.mark.gpu
def test_batch_created_again_on_the_same_solver(opts, room):
    """a batch of three streams, stepped, then a batch of two on the same solver (the first one's buffers are released through the records): it behaves like a batch
    created fresh"""
    scan = room[2]
    fresh_s, fresh = _batch(opts, room, 2)
    want = [_step(fresh, scan[k]) for k in (0, 1)]
    fresh_s.close()
    s, b = _batch(opts, room, 3)
    _step(b, scan[0])
    _, b2 = _batch(opts, room, 2, solver=s)
    assert [_step(b2, scan[k]) for k in (0, 1)] == want
    s.close()
