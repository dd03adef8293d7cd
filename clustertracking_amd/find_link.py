"""Find and link with relocation: the reference's ``find_link`` (find_link.py:914-1041, the loop of
``FindLinker.assign_links``, :869-911, with ``Subnets.merge_lost_subnets``, :329-370) on the MI355X
(``ctr_find_link_device``).

The features of every frame are located and characterised as :func:`find.locate` does, then linked
level by level; where a sub-network has fewer destinations than sources the frame is searched again
around the lost features (the rule of ``relocate.relocate_arrays``) and what is found is offered to
the linker, so a feature that the location misses in a frame keeps its track.  The whole loop is
queued on the device: positions, candidates and frames do not come back to the host in between.
There is no CPU fallback.

Not the reference's on every input: the short sub-networks of a level do not see each other's
claimed candidates (the reference adds them to the background of the queries it issues later), so
on a *coupled* level -- reported per level, see :func:`find_link_arrays` -- parity with the reference
is not pinned.

``refine=True`` is the reference's convenience parameter (find_link.py:436-465): after every level
its features, the relocated ones included, are moved to their centre of mass in the RAW frame
(``ctr_find_link_refine_device``; the rule of ``refine_com.refine_com_arrays``), and the linker
measures the next level from the refined positions, so a track is kept or lost differently than
with whole-pixel sources.  The rule is trackpy's ``refine_com`` restated, with a clip at the edge of
the frame that trackpy lacks: parity with trackpy itself is not pinned, the loop around it is the
reference's.  ``before_link`` and ``after_link`` (Python per frame) and a callable ``refine`` are
not taken.
"""
import collections

import numpy as np
import pandas as pd

from . import _abi, _lib
from ._lib import EngineError
from .find import _characterize_device, _device_frames, _size_columns, locate_arrays
from .link import SubnetOversizeException
from .refine_com import MAX_ITERATIONS, SHIFT_THRESH, descriptor as _refine_descriptor
from .utils import validate_tuple

MAX_QUERIES = 64        # relocation queries per level (short sub-networks after merging)
MAX_RELOCATED = 64      # relocated rows per level

FindLinkResult = collections.namedtuple(
    'FindLinkResult', 'pos frame_offset particle mass signal size relocated n_tracks coupled status')


def _refuse_callbacks(kwargs, refine=False):
    if refine and refine is not True:
        raise NotImplementedError("find_link: a callback is not taken: refine takes True (centre-of-mass "
                                  "refinement after every level) or False")
    for name in ('before_link', 'after_link'):
        if kwargs.pop(name, None):
            raise NotImplementedError("find_link: %s is not taken (a callback per frame): refine=True refines "
                                      "every level by centre of mass, refine_leastsq the result" % name)
    if kwargs:
        raise TypeError("find_link: unexpected arguments %s" % sorted(kwargs))


def find_link_arrays(frames, search_range, separation, diameter=None, memory=0, minmass=0, noise_size=None,
                     smoothing_size=None, threshold=None, percentile=64, device=0, dtype=None,
                     max_queries=MAX_QUERIES, max_relocated=MAX_RELOCATED, scale_factor=1., _on_device=False,
                     refine=False, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH, **kwargs):
    """The arrays behind :func:`find_link`: a ``FindLinkResult`` of NumPy arrays (``_on_device``,
    internal: of torch tensors on the device) --

    ``pos`` float64 [N, ndim] and ``frame_offset`` int64 [T + 1]: rows ``[off[t], off[t + 1])`` are
    the features of frame t, the located rows as ``locate`` orders them, then the relocated rows in
    C order of position; ``particle`` int64 [N]; ``mass``, ``signal`` [N] and ``size`` [N] or
    [N, ndim]; ``relocated`` bool [N]; ``n_tracks``; ``coupled`` bool [T]: a claimed candidate of
    the level lies within the background radius of a source of another short sub-network of the
    level (the reference could decide differently there); ``status`` int32 [4], zeros.  ``pos`` and
    ``frame_offset`` chain into ``refine_leastsq`` / ``link`` / ``motion`` as ``locate``'s do.

    Arguments as :func:`find_link`.  ``max_queries``, ``max_relocated``: the relocation queries and
    the relocated rows one level may have (defaults 64 and 64; 1 .. 1024); ``scale_factor``: what
    the reference reads from the frames' metadata; it divides mass and signal of the relocated rows
    and, without preprocessing (the frames the location looks at are the ones that carry it), of
    the located rows before ``minmass``.
    ``refine=True`` (with ``max_iterations``, ``shift_thresh``: ``refine_com.refine_com_arrays``):
    ``pos`` is sub-pixel, the centre of mass in the raw frame, and ``mass`` the refinement's (the sum
    of the masked raw pixels, no scale factor) for located and relocated rows alike; ``signal`` and
    ``size`` stay from the unrefined position; the relocated rows of a frame follow in C order of
    their refined position.
    Raises ``SubnetOversizeException`` for a sub-network of more than 30 sources after merging and
    ``EngineError`` naming the level for one of more than 64 destinations (relocated included), a
    relocation query beyond ``ctr_relocate_device``'s limits, or a level beyond ``max_queries`` /
    ``max_relocated``; also without a library or a GPU."""
    _refuse_callbacks(kwargs, refine)
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    shape = tuple(frames.shape)
    ndim = len(shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    if int(memory) != memory or memory < 0:
        raise ValueError("memory must be a non-negative integer")
    search_range = validate_tuple(search_range, ndim)
    separation = validate_tuple(separation, ndim)
    # find_link.py:923: the isotropy is that of the diameter AS GIVEN (none given: isotropic)
    isotropic = not hasattr(diameter, '__iter__') or all(d == diameter[0] for d in diameter)
    diameter = separation if diameter is None else validate_tuple(diameter, ndim)
    radius = tuple(int(d // 2) for d in diameter)
    margin = tuple(int(max(d // 2, s // 2 - 1)) for d, s in zip(diameter, separation))
    if any(n <= 2 * m for n, m in zip(shape[1:], margin)):
        raise ValueError("the margin %s leaves nothing of frames of shape %s: use a smaller diameter or "
                         "separation" % (margin, shape[1:]))
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    raw_t, raw_pix = _device_frames(frames, device, dtype)
    dev = raw_t.device
    if noise_size is None:
        proc_t, proc_pix = raw_t, raw_pix
    else:       # find_link.py:957-959, 999: maxima and relocation look at the preprocessed frames
        from . import preprocessing
        if smoothing_size is None:
            smoothing_size = separation
        preprocessing.check_sizes(noise_size, smoothing_size, ndim)
        proc_t, _, proc_pix = preprocessing.preprocess_arrays(raw_t, noise_size, smoothing_size, threshold, device,
                                                              raw_pix, _on_device=True)
    n_frames = int(raw_t.shape[0])
    _, _, pos_i, off, thr = locate_arrays(proc_t, separation, percentile, margin, True, device, proc_pix,
                                          _on_device=True)
    # find_link.py:967: frames that carry a scale factor divide the located rows too; the raw frames
    # of a preprocessed video carry none
    mass, signal, size = _characterize_device(raw_t, pos_i, off, radius, isotropic,
                                              float(scale_factor) if noise_size is None else 1., device, raw_pix)
    nsz = 1 if isotropic else ndim
    with torch.cuda.device(dev):
        # find_link.py:968, 995.  The one place before the loop where a size comes to the host
        rows = torch.nonzero(mass >= minmass).reshape(-1)
        frame_of = torch.repeat_interleave(torch.arange(n_frames, device=dev), off[1:] - off[:-1],
                                           output_size=int(pos_i.shape[0]))
        counts = torch.bincount(frame_of.index_select(0, rows), minlength=n_frames) if n_frames else off[:0]
        loc_off = torch.zeros(n_frames + 1, dtype=torch.int64, device=dev)
        loc_off[1:] = torch.cumsum(counts, 0)
        loc_pos = pos_i.index_select(0, rows).to(torch.float64)
        loc_mass, loc_signal, loc_size = (x.index_select(0, rows) for x in (mass, signal, size))
        m = int(loc_pos.shape[0])
        cap = max(m + max(n_frames - 1, 0) * int(max_relocated), 1)
        out_pos = torch.empty((cap, ndim), dtype=torch.float64, device=dev)
        out_off = torch.zeros(n_frames + 1, dtype=torch.int64, device=dev)
        particle = torch.empty(cap, dtype=torch.int64, device=dev)
        out_mass = torch.empty(cap, dtype=torch.float64, device=dev)
        out_signal = torch.empty(cap, dtype=torch.float64, device=dev)
        out_size = torch.empty((cap, nsz), dtype=torch.float64, device=dev)
        relocated = torch.zeros(cap, dtype=torch.uint8, device=dev)
        n_tracks = torch.zeros(1, dtype=torch.int64, device=dev)
        coupled = torch.zeros(max(n_frames, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        d = _abi.FindLink()
        d.ndim, d.frame_dtype, d.n_frames = ndim, _abi.DTYPE_CODES[np.dtype(proc_pix)], n_frames
        for a in range(ndim):
            d.shape[a] = int(shape[1 + a])
            d.radius[a] = radius[a]
            d.separation[a] = float(separation[a])
            d.search_range[a] = float(search_range[a])
        d.isotropic, d.memory = int(isotropic), int(memory)
        d.max_queries, d.max_relocated = int(max_queries), int(max_relocated)
        d.minmass, d.scale_factor = float(minmass), float(scale_factor)
        d.frames, d.threshold = proc_t.data_ptr(), thr.data_ptr()
        d.n_located = m
        if m:
            d.pos, d.mass, d.signal, d.size = (x.data_ptr() for x in (loc_pos, loc_mass, loc_signal, loc_size))
        d.frame_offset = loc_off.data_ptr()
        d.capacity = cap
        d.pos_out, d.frame_offset_out, d.particle = out_pos.data_ptr(), out_off.data_ptr(), particle.data_ptr()
        d.mass_out, d.signal_out, d.size_out = out_mass.data_ptr(), out_signal.data_ptr(), out_size.data_ptr()
        d.relocated, d.n_tracks, d.coupled, d.status = (x.data_ptr() for x in (relocated, n_tracks, coupled, status))
        if refine:      # find_link.py:462: the refinement reads the raw image
            com = _refine_descriptor(shape[1:], raw_pix, n_frames, radius, max_iterations, shift_thresh)
            com.frames = raw_t.data_ptr()
            eng.on_current_stream(eng.find_link_refine_device, d, com, dev=dev)
        else:
            eng.on_current_stream(eng.find_link_device, d, dev=dev)
        # the one synchronisation of the loop: the status words and the number of rows
        tail = torch.cat([status.to(torch.int64), out_off[-1:]]).cpu()
    code, level, size_seen, _, n = (int(v) for v in tail)
    if code == _abi.FIND_LINK_OVERSIZE:
        raise SubnetOversizeException("Subnetwork contains %d points (level %d)" % (size_seen, level))
    if code != _abi.FIND_LINK_OK:
        what = {_abi.FIND_LINK_CAPACITY: "a sub-network has %d destinations, relocated ones included; the device "
                                         "solver takes %d" % (size_seen, _abi.LINK_MAX_DESTINATIONS),
                _abi.FIND_LINK_RELOCATE: "a relocation query is beyond ctr_relocate_device's per-query limits "
                                         "(status %d)" % size_seen,
                _abi.FIND_LINK_QUERIES: "%d sub-networks look again, max_queries is %d" % (size_seen, max_queries),
                _abi.FIND_LINK_ROWS: "%d relocated rows, max_relocated is %d" % (size_seen, max_relocated),
                }.get(code, "unknown status %d" % code)
        raise EngineError("ctr_find_link_device: level %d: %s" % (level, what))
    res = FindLinkResult(out_pos[:n], out_off, particle[:n], out_mass[:n], out_signal[:n],
                         out_size[:n, 0] if isotropic else out_size[:n], relocated[:n].bool(), n_tracks,
                         coupled[:n_frames].bool(), status)
    if _on_device:
        return res
    return FindLinkResult(*(x.cpu().numpy() for x in res[:7]), int(n_tracks.item()), res.coupled.cpu().numpy(),
                          status.cpu().numpy())


def find_link(frames, search_range, separation, diameter=None, memory=0, minmass=0, noise_size=None,
              smoothing_size=None, threshold=None, percentile=64, device=0, dtype=None, refine=False,
              max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH, **kwargs):
    """Reference ``find_link`` on the MI355X: the features of every frame of ``frames``
    ([T, (z,) y, x], ndarray or tensor on cuda:``device``, as for ``locate``) located, characterised
    and linked, with relocation of the features the location lost.

    Returns a DataFrame with the reference's columns, (z,) y, x, frame, particle, mass, signal,
    size (or size_z / size_y / size_x), and ``relocated``; rows ordered by frame, the located rows
    as ``locate`` orders them, then the relocated rows of the frame in C order of position.
    ``attrs['coupled_levels']`` counts the levels where parity with the reference is not pinned
    (:func:`find_link_arrays`), ``attrs['n_tracks']`` the tracks.

    ``noise_size=None`` (the default here; the reference's is 1) skips the preprocessing.  With it,
    maxima and relocation use the preprocessed frames, which stay on the device; mass, signal and
    size of located rows come from the raw frames, those of relocated rows from the masked
    preprocessed frame (find_link.py:860).  ``refine=True``: the features of every level are moved
    to their centre of mass in the raw frame before the next level is linked (``max_iterations``,
    ``shift_thresh``; :func:`find_link_arrays`); the positions are then sub-pixel and ``mass`` is
    the refinement's.  ``before_link``, ``after_link`` and a callable ``refine`` raise
    ``NotImplementedError``.  Further keywords and the errors: :func:`find_link_arrays`."""
    r = find_link_arrays(frames, search_range, separation, diameter, memory, minmass, noise_size, smoothing_size,
                         threshold, percentile, device, dtype, refine=refine, max_iterations=max_iterations,
                         shift_thresh=shift_thresh, **kwargs)
    ndim = r.pos.shape[1]
    result = pd.DataFrame(r.pos, columns=['z', 'y', 'x'][3 - ndim:])
    result['frame'] = np.repeat(np.arange(len(r.frame_offset) - 1, dtype=np.int64), np.diff(r.frame_offset))
    result['particle'] = r.particle
    result['mass'] = r.mass
    result['signal'] = r.signal
    size = r.size.reshape(len(r.pos), -1)
    for a, key in enumerate(_size_columns(ndim, size.shape[1] == 1)):
        result[key] = size[:, a]
    result['relocated'] = r.relocated
    result.attrs['coupled_levels'] = int(r.coupled.sum())
    result.attrs['n_tracks'] = r.n_tracks
    return result
