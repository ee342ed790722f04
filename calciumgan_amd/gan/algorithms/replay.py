"""Driver of one train() step, eager or as hipGraph replays, for every algorithm.

An algorithm (gan.py, wgan_gp.py) hands over what differs:
  gan._segments(real, rand=None, staged=False) -> [(callable, grad_or_None, wait)]
      the launch segments of one step; the last one leaves the step's seven
      outputs in st['out'].  staged=True: the phase shifts and Adam step sizes
      are read from st['stage_dev'] (the plans' shifts are views of it).
  st['stage_dev']      the staged words of a step on the device (int32)
  gan._fill_stage(host)  fills one pinned slot for the coming step: the shifts,
      drawn in the order of an eager step, then lr_t of every coming Adam step
  gan._adam_steps      Adam steps per train() of (discriminator, generator)
Everything else -- the fixed batch buffer, the staging ring, capture, replay and
the fall-back to eager launches -- is here, once.
"""
import os
import warnings

import torch

# the step replays as hipGraphs after this many eager calls per batch size
GRAPH_WARMUP_CALLS = 2
# pinned staging slots for the host-drawn inputs of a replay: the host may run
# this many steps ahead of the GPU before it waits for a slot's copy
STAGING_SLOTS = 4
# data parallel, A/B only: wait for every gradient all-reduce right after it is
# started instead of overlapping it with the next segment
_DP_OVERLAP = os.environ.get('CALCIUMGAN_DP_OVERLAP', '1') != '0'


def batch_buffer(st, shape, device):
  """The f32 buffer the graphs of state `st` read (or will read) their batch
  from: one per batch size, alive as long as the state."""
  g = st.get('graph')
  if g is not None:
    return g['real']
  if st.get('batch_buf') is None:
    st['batch_buf'] = torch.empty(shape, dtype=torch.float32, device=device)
  return st['batch_buf']


def run_segments(sync, segs):
  """Run (callable, grad, wait) segments -- eager callables or graph replays.
  After a segment with a gradient buffer its all-reduce is STARTED; a segment
  with wait=True needs the pending all-reduce finished first."""
  pending = None
  for fn, grad, wait in segs:
    if wait and pending is not None:
      pending.wait()
      pending = None
    fn()
    if grad is not None:
      pending = sync.all_reduce_async(grad)
      if not _DP_OVERLAP and pending is not None:
        pending.wait()
        pending = None
  if pending is not None:
    pending.wait()


def eager(gan, st, real, rand=None):
  """One step with eager launches; returns the step's output buffer."""
  run_segments(gan._sync, gan._segments(real, rand))
  return st['out']


def _capture(gan, st, real):
  """Capture one train() as hipGraphs, one per segment (RCCL all-reduces stay
  eager between replays, overlapped with the wait=False segments).  Host-drawn
  inputs of a replay are copied to st['stage_dev'] EAGERLY ahead of it, from a
  ring of pinned slots (_stage); z / alpha come from the graph-registered
  device generator."""
  words = st['stage_dev'].numel()
  g = dict(
      # (the caller's own buffer when it gathers its batches into
      # batch_buffer(): no copy in front of a replay then)
      real=(st['batch_buf'] if st.get('batch_buf') is not None and
            st['batch_buf'].shape == real.shape else torch.empty_like(real)),
      # (the f32 words travel as their bit patterns)
      stage_host=[torch.zeros(words, dtype=torch.int32).pin_memory()
                  for _ in range(STAGING_SLOTS)],
      stage_event=[None] * STAGING_SLOTS,
      stage_next=0)
  if g['real'].data_ptr() != real.data_ptr():
    g['real'].copy_(real)
  segs = gan._segments(g['real'], staged=True)
  steps = (gan.dis_optimizer.host_steps, gan.gen_optimizer.host_steps)
  graphs = []
  pool = None
  torch.cuda.synchronize()
  try:
    for fn, grad, wait in segs:
      graph = torch.cuda.CUDAGraph()
      graph.register_generator_state(gan._streams.local)
      # thread_local: the RCCL watchdog thread may touch the HIP runtime
      # while this thread captures
      with torch.cuda.graph(graph, pool=pool, capture_error_mode='thread_local'):
        fn()
      pool = graph.pool()
      graphs.append((graph.replay, grad, wait))
  finally:
    # capture only records: undo the host-side step counters it advanced
    gan.dis_optimizer.host_steps, gan.gen_optimizer.host_steps = steps
  g['graphs'] = graphs
  return g


def _stage(gan, st, g):
  """Host-drawn inputs of the coming replay -> device.  The host writes them
  into the next pinned slot of a ring and enqueues the copy on the launch
  stream (ordered after the previous replay, which still reads the device
  buffer); an event per slot keeps the host from rewriting a slot whose copy
  has not executed yet -- train() never syncs, so the host may run several
  steps ahead of the GPU."""
  k = g['stage_next']
  g['stage_next'] = (k + 1) % STAGING_SLOTS
  if g['stage_event'][k] is not None:
    g['stage_event'][k].synchronize()
  host = g['stage_host'][k]
  gan._fill_stage(host)
  st['stage_dev'].copy_(host, non_blocking=True)
  ev = g['stage_event'][k] = torch.cuda.Event()
  ev.record()


def replay(gan, st, real):
  """One step as graph replays (captured on the first call; st['graph'] is
  None until then); returns the step's output buffer."""
  g = st.get('graph')
  if g is None:
    try:
      g = st['graph'] = _capture(gan, st, real)
    except Exception as e:  # noqa: BLE001 -- any capture failure
      # the step itself is unaffected: keep training with eager launches
      warnings.warn('calciumgan_amd: hipGraph capture of train() failed '
                    '({}: {}); continuing with eager launches'.format(
                        type(e).__name__, e))
      gan._use_graph = False
      torch.cuda.synchronize()
      return eager(gan, st, real)
  # the graphs read their batch from a fixed buffer.  A caller that gathers
  # its batches into batch_buffer() wrote it already; any other tensor is
  # copied (107 MB at cfg2, ~35 us; 4.3 GB at cfg5, 2 ms)
  if g['real'].data_ptr() != real.data_ptr():
    g['real'].copy_(real)
  # (the draw order of an eager step: z / alpha on the device generator inside
  # the graphs, the shifts here)
  _stage(gan, st, g)
  run_segments(gan._sync, g['graphs'])
  gan.dis_optimizer.host_steps += gan._adam_steps[0]
  gan.gen_optimizer.host_steps += gan._adam_steps[1]
  return st['out']
