"""GPU: the SIFT front end keeps device state between calls - the HIP graphs ``pano_sift_detect``
captures, the context's list of scale-space extrema (grown when a frame needs more), the workspace
rings of ``features.SiftPipeline`` and the engine's ring of pinned counters.  Here frame sizes mix
on one engine, in an order that grows the extrema list after graphs were captured, and results are
taken late or kept while later frames go through the same ring.  Every detection is compared with
the same frame detected launch by launch (``OPT_SIFT_GRAPH`` = 0) on an engine of its own
(tests/sift_reference.py: keypoints, angles and descriptors bit for bit - the histograms are sums
of integer fixed-point votes, independent of the atomics' order)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sift_reference import assert_same_detection  # noqa: E402

pytestmark = pytest.mark.gpu

# (h, w): below the extrema list's floor of 1 << 20 entries, 2.07 M and 8.29 M entries
S, M, L = (200, 320), (1080, 1920), (2160, 3840)
# runs of (size, frames): S's graph is captured and replayed, then M grows the list; both replay
# again, then L grows it past both
RUNS = [(S, 3), (M, 1), (S, 3), (M, 3), (L, 1), (M, 3), (S, 3), (L, 3)]


class Frames:
    """Device frames ``synth.make_frame(seed, w, h, "B")`` and their reference detections (host
    keypoints, host descriptors), made once per module."""

    def __init__(self, eng):
        from pano360_amd import _lib, engine
        self.device = eng.device
        self.ref = engine.Engine(eng.device)
        self.ref.set_option(_lib.OPT_SIFT_GRAPH, 0)
        self.frames, self.refs, self.pipes = {}, {}, {}

    def frame(self, size, seed):
        import torch
        from pano360_amd import synth
        key = (size, seed)
        if key not in self.frames:
            h, w = size
            self.frames[key] = torch.from_numpy(synth.make_frame(seed, w, h, "B")).to(self.device)
            torch.cuda.synchronize(self.device)
        return self.frames[key]

    def reference(self, size, seed):
        from pano360_amd import features
        key = (size, seed)
        if key not in self.refs:
            if size not in self.pipes:
                self.pipes[size] = features.SiftPipeline(self.ref, *size, depth=1)
            kps, desc = self.pipes[size].detect(self.frame(size, seed)).result()
            assert len(kps) > 15
            self.refs[key] = (kps, desc.cpu().numpy())
        return self.refs[key]

    def prepare(self, frames):
        """Every (size, seed) frame and its reference made now: nothing waits for the device later."""
        for size, seed in frames:
            self.reference(size, seed)
        import torch
        torch.cuda.synchronize(self.device)

    def check(self, result, size, seed):
        kps, desc = result
        assert_same_detection(kps, desc, *self.reference(size, seed))


@pytest.fixture(scope="module")
def frames(eng):
    return Frames(eng)


def graph_engine(eng):
    """A fresh engine (context, graphs, extrema list of its own) that replays graphs."""
    from pano360_amd import _lib, engine
    use = engine.Engine(eng.device)
    use.set_option(_lib.OPT_SIFT_GRAPH, 1)
    return use


def schedule():
    """RUNS as [[(size, seed, grows)] per run]: three frames per size, taken in turn; ``grows``: the
    frame needs a longer extrema list than every frame before it on one context."""
    cap, count, runs = 0, {}, []
    for size, n in RUNS:
        run = []
        for _ in range(n):
            need = max(size[0] * size[1], 1 << 20)
            run.append((size, 10 * size[0] + count.get(size, 0) % 3, cap > 0 and need > cap))
            count[size] = count.get(size, 0) + 1
            cap = max(cap, need)
        runs.append(run)
    return runs


def test_graph_replay_survives_extrema_list_growth(eng, frames):
    """One engine, one depth-1 pipeline per size, the frames of RUNS on two torch streams taken in
    turn (each step ordered after the one before: one context has one extrema list).  A frame's
    result is taken only when the next frame has been queued - at a growth frame, the replays
    before it are still in flight when the list is freed and reallocated.  Every result equals the
    reference; every run of three ends replaying; and the first frame of a size after a growth does
    not replay the graph captured before it (that graph holds the old list)."""
    import torch
    from pano360_amd import features
    runs = schedule()
    frames.prepare((size, seed) for run in runs for size, seed, _ in run)
    use = graph_engine(eng)
    streams = [torch.cuda.Stream(eng.device) for _ in range(2)]
    prev = torch.cuda.current_stream(eng.device)
    pipes, pending = {}, {}
    stale, k = set(), 0             # stale: sizes with a graph from before the latest growth

    def settle(size):
        det, seed = pending.pop(size)
        frames.check(det.result(), size, seed)

    for run in runs:
        for size, seed, grows in run:
            if size not in pipes:
                pipes[size] = features.SiftPipeline(use, *size, depth=1)
            if size in pending:     # (depth 1: this frame takes the workspace)
                settle(size)
            stream = streams[k % 2]
            stream.wait_stream(prev)
            with torch.cuda.stream(stream):
                det = pipes[size].detect(frames.frame(size, seed))
            prev, k = stream, k + 1
            if grows:
                stale = set(pipes) - {size}
            elif size in stale:
                assert not pipes[size].replaying, f"frame {k}: a graph from before the growth replayed"
                stale.discard(size)
            for other in [s for s in pending if s != size]:
                settle(other)
            pending[size] = (det, seed)
        if len(run) == 3:
            assert pipes[size].replaying, f"frame {k}: a run of three ended without replaying"
    for size in list(pending):
        settle(size)
    torch.cuda.synchronize()


def test_engine_pipeline_mixes_three_frame_sizes(eng, frames):
    """The frames of RUNS through the public ``features.sift_detect_device`` on one engine, on two
    streams taken in turn as above.  The engine keeps pipelines of two frame sizes: the third size
    drops one, which is made again later (perhaps in the very buffers it had: the caching allocator
    hands them back) - its graphs of before may match again, but only if the extrema list is the
    one they were captured with.  Every result equals the reference."""
    import torch
    from pano360_amd import features
    runs = schedule()
    frames.prepare((size, seed) for run in runs for size, seed, _ in run)
    use = graph_engine(eng)
    streams = [torch.cuda.Stream(eng.device) for _ in range(2)]
    prev = torch.cuda.current_stream(eng.device)
    k = 0
    for run in runs:
        for size, seed, _ in run:
            stream = streams[k % 2]
            stream.wait_stream(prev)
            with torch.cuda.stream(stream):
                got = features.sift_detect_device(frames.frame(size, seed), eng=use)
                frames.check(got, size, seed)
            prev, k = stream, k + 1
            assert len(use._sift_pipelines) <= 2
    torch.cuda.synchronize()


def test_public_detections_own_their_results(eng, frames):
    """Six frames of one size through ``sift_detect_device``, every (keypoints, descriptors) kept
    on the device, then three more detections of that size on the same engine (the pipeline's
    three workspaces go round once more): all six still equal their references."""
    import torch
    from pano360_amd import features
    seeds = [500 + i for i in range(9)]
    frames.prepare((S, seed) for seed in seeds)
    use = graph_engine(eng)
    kept = [features.sift_detect_device(frames.frame(S, seed), eng=use) for seed in seeds[:6]]
    for seed in seeds[6:]:
        frames.check(features.sift_detect_device(frames.frame(S, seed), eng=use), S, seed)
    for got, seed in zip(kept, seeds[:6]):
        frames.check(got, S, seed)
    torch.cuda.synchronize()


def test_a_recycled_slot_is_not_read(eng, frames):
    """``SiftPipeline(depth=2)``: three detections queued without a result taken - the first one's
    workspace has gone to the third, so its ``result()`` raises instead of returning the third
    frame's lists under its own counts; the other two equal their references.  A result taken
    before its workspace was reused keeps its keypoints (a host copy; an explicit pipeline's
    descriptors are a view into the ring and are not the caller's)."""
    import torch
    from pano360_amd import _lib, features
    seeds = [600 + i for i in range(4)]
    frames.prepare((S, seed) for seed in seeds)
    use = graph_engine(eng)
    pipe = features.SiftPipeline(use, *S, depth=2)
    early = pipe.detect(frames.frame(S, seeds[0]))
    kps_early = early.result()[0]
    dets = [pipe.detect(frames.frame(S, seed)) for seed in seeds[1:]]
    with pytest.raises(_lib.PanoError):
        dets[0].result()
    for det, seed in zip(dets[1:], seeds[2:]):
        frames.check(det.result(), S, seed)
    kps_ref = frames.reference(S, seeds[0])[0]
    for kps in (kps_early, early.result()[0]):
        assert len(kps) == len(kps_ref)
        for key in ("x", "y", "size", "response", "octave", "r", "c"):
            assert np.array_equal(kps[key], kps_ref[key]), key
    torch.cuda.synchronize()


def test_results_taken_a_frame_late_on_a_three_deep_ring(eng, frames):
    """``bench.py --workload cfg4 --detect``'s loop: nine frames on ``SiftPipeline(depth=3)``, each
    result taken when the next frame has been queued - none raises, all equal their references."""
    import torch
    from pano360_amd import features
    seeds = [700 + i % 4 for i in range(9)]
    frames.prepare((S, seed) for seed in seeds)
    use = graph_engine(eng)
    pipe = features.SiftPipeline(use, *S, depth=3)
    job = None
    for seed in seeds:
        det = pipe.detect(frames.frame(S, seed))
        if job is not None:
            frames.check(job[0].result(), S, job[1])
        job = (det, seed)
    frames.check(job[0].result(), S, job[1])
    assert pipe.replaying
    torch.cuda.synchronize()


def test_a_recycled_counter_slot_is_not_read(eng, frames):
    """The engine's ring of pinned counter slots is shorter than a deep pipeline: seventeen
    detections queued and finished, then every result taken - the first one's slot holds the
    seventeenth's counts by then, and its result still has its own frame's keypoints."""
    import torch
    from pano360_amd import features
    seeds = [800 + i % 3 for i in range(features._SiftHost.SLOTS + 1)]
    frames.prepare((S, seed) for seed in seeds)
    # (the first and the last frame share a slot: their counts must differ for the test to see it)
    assert len(frames.reference(S, seeds[0])[0]) != len(frames.reference(S, seeds[-1])[0])
    use = graph_engine(eng)
    pipe = features.SiftPipeline(use, *S, depth=len(seeds), max_keypoints=1 << 14)
    dets = [pipe.detect(frames.frame(S, seed)) for seed in seeds]
    torch.cuda.synchronize()        # the last frame's counts have landed in the shared slot
    for det, seed in zip(dets, seeds):
        frames.check(det.result(), S, seed)
    torch.cuda.synchronize()
