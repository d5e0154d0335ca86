"""Captured learner steps: one hipGraph (or two, around the data-parallel split point) per key, each with its own
static input buffers, all captured on one stream by one procedure."""
from __future__ import annotations

import itertools
import threading

import torch


# Held while the learner captures a step graph: background threads of the learner process (the ingest stager's
# rare buffer growth) take it around their pinned / device allocations, so no allocation from another thread lands
# inside a capture window (HIP invalidates a capture on some cross-thread API calls even in thread-local mode).
CAPTURE_LOCK = threading.RLock()

# Only the capturing thread's HIP calls are capture-checked: other threads of the process keep running while the
# learner captures — RCCL's watchdog querying events, or an in-process actor stepping its own graphs on its own
# streams (learner/e2e.py). Neither touches the capturing stream.
CAPTURE_ERROR_MODE = 'thread_local'

_TOKENS = itertools.count(1)
_TOKEN_ATTR = '_dca_graph_token'


class StepGraphs:
    """key → (graphs, the body's returned tensors, the key's static inputs)."""

    def __init__(self, device):
        self.device = device
        self._stream = None     # the capture stream: lives as long as the cache, so it outlives the graphs made on it
        self._steps = {}
        self.last = None        # the most recently captured graph (None before any capture / once released)

    def __len__(self):
        return len(self._steps)

    def __iter__(self):
        return iter(self._steps)

    def static(self, key):
        """The static inputs the graphs of ``key`` read."""
        return self._steps[key][2]

    @staticmethod
    def replay_key(replay, B: int, S: int):
        """Key of a replay source. A token unique for the object's lifetime, never ``id()``: a later pool allocated
        at a freed pool's address must not find (and replay) a graph wired to the freed storage."""
        tok = replay.__dict__.get(_TOKEN_ATTR)
        if tok is None:
            tok = replay.__dict__[_TOKEN_ATTR] = next(_TOKENS)
        return ('replay', tok, B, S)

    def release(self, replay) -> int:
        """Drop every captured step (graphs, their private memory pool and static inputs) bound to ``replay``;
        returns how many."""
        tok = replay.__dict__.get(_TOKEN_ATTR)
        dead = [k for k in self._steps if tok is not None and k[0] == 'replay' and k[1] == tok]
        for k in dead:
            if self.last in self._steps.pop(k)[0]:
                self.last = None
        return len(dead)

    def step(self, key, make_static, fill, body, between=None):
        """Run the captured step of ``key``. A new key gets its static inputs from ``make_static()`` and
        ``body(static, hook)`` is captured reading them; a known key has this step's inputs written by
        ``fill(static)``. ``between`` asks for a split step: replayed as graph 1, ``between()``, graph 2."""
        step = self._steps.get(key)
        if step is None:
            static = make_static()
            graphs, out = self._capture(lambda hook: body(static, hook), split=between is not None)
            step = self._steps[key] = (graphs, out, static)
            self.last = graphs[0]
        else:
            fill(step[2])
        graphs, out, _ = step
        graphs[0].replay()
        if between is not None:
            between()
            graphs[1].replay()
        return out

    def _capture(self, body, split: bool):
        """Capture ``body(hook)``. A step that calls its hook ends the running capture there and begins the next
        graph in the first graph's memory pool; one that never does yields one graph."""
        if self._stream is None:
            # default priority: high priority measured slower (profiles/r4_stream_priority_ab.txt)
            self._stream = torch.cuda.Stream(device=self.device)
        s, cur = self._stream, torch.cuda.current_stream(self.device)
        s.wait_stream(cur)
        with torch.cuda.stream(s):      # one eager run on the capture stream (allocator warm-up), no collectives
            body(lambda: None)
        cur.wait_stream(s)
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()     # (made outside the capture window)
        graphs = [g1]

        def switch():
            g1.capture_end()
            g2.capture_begin(pool=g1.pool(), capture_error_mode=CAPTURE_ERROR_MODE)
            graphs.append(g2)

        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()        # (as torch.cuda.graph does: the warm-up's blocks go back before the pool grows)
        with CAPTURE_LOCK, torch.cuda.stream(s):
            g1.capture_begin(capture_error_mode=CAPTURE_ERROR_MODE)
            out = body(switch)
            if split and len(graphs) == 1:
                raise RuntimeError('direct step never reached its DP split point')
            graphs[-1].capture_end()
        cur.wait_stream(s)
        return tuple(graphs), out
