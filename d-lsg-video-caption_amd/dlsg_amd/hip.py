"""ctypes binding of libdlsg_hip.so -- the only device compute path of this package.  The argument structs, the prototypes and
the DLSG_* constants are not written down here: dlsg_amd/abi.py reads them from include/dlsg.h, and this module refers to a
struct by its header name (abi.dlsg_gemm_args).

There is no CPU or eager-PyTorch fallback here: constructing `HipOps` raises if the library is missing or no
MI355X is visible.  Tensors are only device memory + strides; every op is a hand-written HIP kernel launched on
PyTorch's current HIP stream.

All methods take torch *views*: 2-d (rows, cols) with unit inner stride and an arbitrary row stride, or 3-d
(batch, rows, cols) for batched GEMMs (the batch stride may be 0 via .expand()).
"""
import ctypes as C
import math
import os

import torch

from . import abi, limits

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdlsg_hip.so')

# numeric aliases of the header's #defines: a value cannot disagree with include/dlsg.h, a renamed define is a KeyError here
_D = abi.defines
ABI_VERSION = _D['DLSG_ABI_VERSION']
MAXG = _D['DLSG_GEMM_MAXG']
SAMPLE_FILTER_MAXV = _D['DLSG_SAMPLE_FILTER_MAXV']
GEMM_NT, GEMM_NN, GEMM_TN = _D['DLSG_GEMM_NT'], _D['DLSG_GEMM_NN'], _D['DLSG_GEMM_TN']
F_ACCUM, F_BIAS, F_TANH = _D['DLSG_GEMM_ACCUM'], _D['DLSG_GEMM_BIAS'], _D['DLSG_GEMM_TANH']
F_FORCE64, F_FORCE128, F_TILE256, F_BF16X3 = (_D['DLSG_GEMM_' + n] for n in ('FORCE64', 'FORCE128', 'TILE256', 'BF16X3'))
F_SK, F_NOSK, F_SK_BM128, F_SK_BM256, F_SK_BN128, F_SK_NOXMAP = (_D['DLSG_GEMM_' + n] for n in (
    'SK', 'NOSK', 'SK_BM128', 'SK_BM256', 'SK_BN128', 'SK_NOXMAP'))
GRAD_SUMSQ_SLOTS = _D['DLSG_GRAD_SUMSQ_SLOTS']   # float64 partials one dlsg_grad_sumsq launch writes
CLIP_NORM, CLIP_COEF, CLIP_NONFINITE, CLIP_RECORD_FLOATS = (_D['DLSG_CLIP_' + n] for n in ('NORM', 'COEF', 'NONFINITE', 'RECORD_FLOATS'))
ADAM_MAX_RANGES = _D['DLSG_ADAM_MAX_RANGES']     # decayed intervals one dlsg_adamw_ema launch takes
ENS_MAX = _D['DLSG_ENS_MAX']                    # members dlsg_beam_select_ens combines
METRICS_STAGE = _D['DLSG_METRICS_STAGE']        # reference words dlsg_caption_metrics stages in LDS per pass
F_SK_GIVEAWAY = _D['DLSG_GEMM_SK_GIVEAWAY']   # test hook (include/dlsg.h): the split tiles are finished by their last contributor alone

i64, u32, u64, f32 = C.c_int64, C.c_uint32, C.c_uint64, C.c_float


def load_library(path=LIB_PATH):
    """libdlsg_hip.so with the argtypes and restype of every entry point include/dlsg.h, the extension headers beside it and the
    headers under include/addons/ declare (dlsg_amd/abi.py reads them)"""
    if not os.path.exists(path):
        raise RuntimeError('libdlsg_hip.so not built (%s): run `python -c "import __graft_entry__ as g; g.build()"` '
                           'or `make -C d-lsg-video-caption_amd/csrc`; there is no fallback path' % path)
    lib = C.CDLL(path)
    for name, (restype, argtypes) in list(abi.functions.items()) + list(abi.extensions.items()) + list(abi.addons.items()):
        fn = getattr(lib, name)  # AttributeError if the library does not export what a header declares
        fn.restype, fn.argtypes = restype, argtypes
    if lib.dlsg_abi_version() != ABI_VERSION:
        raise RuntimeError('libdlsg_hip.so ABI mismatch: library %d, include/dlsg.h %d (rebuild: make -C d-lsg-video-caption_amd/csrc)'
                           % (lib.dlsg_abi_version(), ABI_VERSION))
    return lib




def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chkc(t):
    if not t.is_contiguous():
        raise ValueError('fused decoder-step kernels take dense row-major buffers')


def _seed(seed):
    """seed is an int, or a 1-element int64 device tensor (graph mode: the kernels read it at run time)."""
    if torch.is_tensor(seed):
        return 0, C.c_void_p(seed.data_ptr())
    return int(seed), None


def cider_tables(tb):
    """the dlsg_cider_tables of a scoring.DeviceCiderD (device pointers; an empty table is NULL)"""
    def p(t):
        return t.data_ptr() if t.numel() else None
    return abi.dlsg_cider_tables(p(tb.gram_keys), p(tb.gram_idf), p(tb.clip_off), p(tb.ref_off), p(tb.ref_norm), p(tb.ref_len),
                                 p(tb.ent_keys), p(tb.ent_w), tb.gram_keys.numel(), tb.log_n, tb.sigma, tb.n_clips, tb.V, tb.n, 0)


def host_to_device(values, dtype, device):
    """A small host array (per-step scalars: coins, seeds, Adam's bias corrections, caption lengths, gather indices) as a device
    tensor WITHOUT stalling the host.  A copy from pageable memory is synchronous on ROCm -- it waits until the stream has run dry --
    so a loop that sends three scalars per step never gets ahead of the device, and every microsecond of host work between two
    steps is device idle time (bench.py `sustained`: 0.8 ms per step).  Staged through the caching pinned allocator the copy is
    enqueued and the host moves on; the allocator keeps the block until the copy's event has passed."""
    t = values.to(dtype) if torch.is_tensor(values) else torch.as_tensor(values, dtype=dtype)
    device = torch.device(device)
    if device.type != 'cuda' or t.is_cuda:
        return t.to(device)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def copy_to_device(dst, values, dtype=None):
    """dst (device tensor) <- values, same staging as `host_to_device`"""
    t = values.to(dtype or dst.dtype) if torch.is_tensor(values) else torch.as_tensor(values, dtype=dtype or dst.dtype)
    if dst.is_cuda and not t.is_cuda:
        t = t.contiguous().pin_memory()
    dst.copy_(t.view(dst.shape), non_blocking=True)


def normalised_weights(weights):
    """the members' weights of `beam_select_ens` as the kernel gets them: w / sum(w) in float64 (a list of Python floats)"""
    w = [float(x) for x in weights]
    if not w or not all(math.isfinite(x) and x > 0.0 for x in w):
        raise ValueError('ensemble weights must be finite and positive, not %r' % (list(weights),))
    tot = math.fsum(w)
    return [x / tot for x in w]


def _chk2(t):
    assert t.dim() == 2 and (t.stride(1) == 1 or t.size(1) == 1) and t.dtype == torch.float32, (t.shape, t.stride())
    return t


class HipOps(object):
    """Launches the HIP kernels on torch's current stream.  Raises if the library or the GPU is missing."""

    name = 'hip'

    def __init__(self):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError('dlsg_amd needs an MI355X (gfx950) device: torch.cuda.is_available() is False and '
                               'there is no CPU fallback')
        self.prof = None          # set to {} by bench.py: key -> list of (start event, end event, algorithmic work)
        self.extra_flags = 0      # OR-ed into every dlsg_gemm call (precision policy: F_BF16X3), set by the model
        self.prof_min_flops = 2e9  # dlsg_gemm calls below this are not bracketed by profile events (tools/pmc_step_target.py: 0)
        self.flop_count = None     # a float: every dlsg_gemm call adds its 2 M N K (bench.py: executed flops of a step)
        self._tail_ws = {}         # device -> workspace of dec_tail_fwd's split vocabulary scan (_dec_tail_ws)

    # ------------------------------------------------------------------ live per-kernel timing (bench.py roofline)
    def _prof_begin(self):
        if self.prof is None:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def _prof_end(self, key, e0, work, shape='', operand_bytes=None):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.prof.setdefault(key, []).append((e0, e1, work, shape, operand_bytes))

    def prof_summary(self):
        """key -> dict(launches, ms_total, work_total, shapes: launch shape -> the same three); call after
        torch.cuda.synchronize().  A kernel symbol runs several launch shapes in a step; traffic counters are per shape."""
        out = {}
        for key, rec in (self.prof or {}).items():
            shapes, samples = {}, {}
            for a, b, w, shp, ob in rec:
                d = shapes.setdefault(shp, dict(launches=0, ms_total=0.0, work_total=0.0, operand_bytes=ob))
                d['launches'] += 1; d['work_total'] += float(w)
                samples.setdefault(shp, []).append(a.elapsed_time(b))
            # a shape's time = launches x the MEDIAN of its samples: the span between two events also holds whatever the host
            # took to issue the launch while the device sat idle (the first launch of an eager step: one sample of 10 ms among
            # three turned a 0.2-ms launch into "3.6 ms" in one run)
            for shp, ms in samples.items():
                ms = sorted(ms)
                med = ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2])
                shapes[shp]['ms_total'] = med * len(ms)
            out[key] = dict(launches=len(rec), ms_total=sum(d['ms_total'] for d in shapes.values()),
                            work_total=float(sum(r[2] for r in rec)), shapes=shapes)
        return out

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    launches = 0              # entry-point calls made through this binding (bench.py: launches per decode step)

    def _check(self, rc, what):
        self.launches += 1
        if rc != 0:
            raise RuntimeError('%s failed with code %d' % (what, rc))

    # ------------------------------------------------------------------ GEMM
    stream_k = True           # False: dlsg_gemm gets no workspace, so every product runs on the tiled kernels
    sk_cu_budget = 0          # > 0: stream-K launches use at most this many workgroups (dlsg_gemm_args.cu_budget): the backward of a
                              # Trainer with several ranks leaves CUs to the bucket all-reduces that run beside it

    # process-wide (class attributes): launches on one stream are serialised, so every model, trainer and captured graph that
    # launches on a stream can share that stream's workspace; captures all run on ONE side stream per device (capture_stream), so a
    # process holds two workspaces per device (~134 MB each on 256 CUs), not one per captured graph
    _gemm_ws = {}
    _capture_streams = {}

    @classmethod
    def capture_stream(cls, dev):
        """the side stream every hipGraph capture of this process runs on -- graphs.capture_segments takes it for all seven capture
        sites: the Trainer's step, the GanTrainer's critic update and generator term, GreedyGraph, SampleGraph, BeamGraph and
        NBestBeamGraph.  Captures are sequential and replays go to the caller's current stream, so one stream -- and one stream-K
        workspace, warmed by the eager pass that precedes every capture -- serves them all"""
        dev = torch.device(dev)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        st = cls._capture_streams.get(idx)
        if st is None:
            st = cls._capture_streams[idx] = torch.cuda.Stream(device=idx)
        return st

    def _gemm_workspace(self, dev):
        """the stream-K kernel's scratch (csrc/gemm_sk.hip): counters + two accumulator slots per CU, zero-filled once; one per
        (device, stream), because two launches that may overlap must not share it.  None while a capture is running on a stream
        that has no workspace yet (no allocation + fill inside a capture): the call then runs on the tiled kernels."""
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = HipOps._gemm_ws.get(key)
        if ws is None:
            n = int(self.lib.dlsg_gemm_ws_bytes())
            if n <= 0:
                raise RuntimeError('dlsg_gemm_ws_bytes() failed: no device?')
            if torch.cuda.is_current_stream_capturing():
                return None
            ws = HipOps._gemm_ws[key] = torch.zeros((n + 3) // 4, dtype=torch.float32, device=dev)
        return ws

    def device_cus(self):
        """compute units of the current device (what a stream-K launch fills: the workspace is two slots per CU)"""
        n = int(self.lib.dlsg_gemm_ws_bytes())
        return max(0, (n - 16384) // (2 * 256 * 256 * 4))

    def comm_rehearsal(self, view, workgroups, passes):
        """one-GPU stand-in for the footprint of a ring all-reduce over `view` (dlsg_comm_rehearsal), on the current stream"""
        self._check(self.lib.dlsg_comm_rehearsal(_p(view), i64(view.numel()), int(workgroups), int(passes), self._stream()),
                    'dlsg_comm_rehearsal')

    def gemm(self, mode, groups, alpha=1.0, flags=0, bias=None, skip_if=None, plan_only=False):
        """groups: list of (A, B, C[, bias]) views (2-d, or 3-d batched with identical batch strides across groups).
        plan_only: nothing is launched; returns the tile family the library would run the call on (dlsg_gemm_variant)."""
        a = abi.dlsg_gemm_args()
        A0, B0, C0 = groups[0][:3]
        batched = A0.dim() == 3
        if batched:
            nb = C0.size(0)
            a.bsa, a.bsb, a.bsc = A0.stride(0), B0.stride(0), C0.stride(0)
        else:
            nb = 1
            a.bsa = a.bsb = a.bsc = 0
        M = C0.shape[-2]
        N = max(g[2].shape[-1] for g in groups)          # groups may write column blocks of different widths
        a.mode, a.M, a.N, a.ldc = mode, M, N, C0.stride(-2)
        a.ngroups, a.nbatch, a.alpha = len(groups), nb, alpha
        gbias = any(len(g) > 3 and g[3] is not None for g in groups)
        a.flags = flags | self.extra_flags | (F_BIAS if (bias is not None or gbias) else 0)
        a.bias = _p(bias)
        a.skip_if = _p(skip_if)          # 1-element int32 device tensor: launch is a no-op when it is non-zero
        if (self.stream_k or (flags & F_SK)) and not ((flags | self.extra_flags) & F_NOSK):
            ws = self._gemm_workspace(C0.device)
            if ws is not None:
                a.ws, a.ws_bytes = _p(ws), ws.numel() * 4
                a.cu_budget = int(self.sk_cu_budget)
        assert len(groups) <= MAXG
        for i, grp_ in enumerate(groups):
            A, B, Cc = grp_[:3]
            Ng = Cc.shape[-1]
            if mode == GEMM_TN:
                K = A.shape[-2]
                assert A.shape[-1] == M and B.shape[-2] == K and B.shape[-1] == Ng, (A.shape, B.shape, Cc.shape)
            elif mode == GEMM_NN:
                K = A.shape[-1]
                assert A.shape[-2] == M and B.shape[-2] == K and B.shape[-1] == Ng, (A.shape, B.shape, Cc.shape)
            else:
                K = A.shape[-1]
                assert A.shape[-2] == M and B.shape[-1] == K and B.shape[-2] == Ng, (A.shape, B.shape, Cc.shape)
            for t in (A, B, Cc):
                assert t.dtype == torch.float32 and (t.stride(-1) == 1 or t.size(-1) == 1), (t.shape, t.stride())
            assert Cc.shape[-2] == M
            if batched:
                assert (A.stride(0), B.stride(0), Cc.stride(0)) == (a.bsa, a.bsb, a.bsc)
            g = a.g[i]
            g.A, g.B, g.C = _p(A), _p(B), _p(Cc)
            g.lda, g.ldb, g.K, g.N = A.stride(-2), B.stride(-2), K, (Ng if Ng != N else 0)
            g.bias = _p(grp_[3]) if len(grp_) > 3 else None
            g.ldc = Cc.stride(-2) if Cc.stride(-2) != a.ldc else 0
        if plan_only:
            return int(self.lib.dlsg_gemm_variant(C.byref(a)))
        e0 = None
        if self.flop_count is not None:
            self.flop_count += 2.0 * M * nb * sum(grp_[2].shape[-1] * a.g[i].K for i, grp_ in enumerate(groups))
        if self.prof is not None:
            flops = 2.0 * M * nb * sum(grp_[2].shape[-1] * a.g[i].K for i, grp_ in enumerate(groups))     # (groups of different widths)
            if flops >= self.prof_min_flops:     # only the heavy launches are timed, so the events do not perturb the step
                e0 = self._prof_begin()
        self._check(self.lib.dlsg_gemm(C.byref(a), self._stream()), 'dlsg_gemm')
        if e0 is not None:
            x3 = bool(a.flags & F_BF16X3)
            if x3:
                # the split-bf16 dispatch rule (csrc/gemm_bf16x3.hip)
                tiles_l = ((M + 127) // 128) * ((N + 127) // 128) * nb * len(groups)
                if a.flags & (F_FORCE64 | F_FORCE128):
                    variant = '64x64' if a.flags & F_FORCE64 else '128x128'
                elif M <= 64 and mode != GEMM_TN and N >= 64:
                    variant = 'skinny_64x32'
                else:
                    variant = '128x128' if tiles_l >= 1000 else '64x64'
            else:
                v = self.lib.dlsg_gemm_variant(C.byref(a))         # the library's own answer (csrc/gemm.hip, gemm_plan)
                variant = {0: '64x64', 1: '128x64', 2: '128x128', 3: 'skinny_64x32' if M <= 64 else 'skinny_128x32', 4: '256x256',
                           5: '256x128', 6: '256x256+rest', 7: 'streamk_256x256'}[v]
            # one key per kernel symbol (arithmetic, tile, operand layout), as rocprofv3 --stats lists them
            ks = sorted(set(a.g[i].K for i in range(len(groups))))
            ns_ = sorted(set(grp_[2].shape[-1] for grp_ in groups))
            shape = '%s M=%d N=%s K=%s groups=%d batch=%d' % (('NT', 'NN', 'TN')[mode], M, '/'.join(map(str, ns_)), '/'.join(map(str, ks)),
                                                              len(groups), nb)
            # bytes of the operands and results of one launch, every group's counted on its own (groups that share an operand --
            # the two streams' region projections read the same regions -- make the unique bytes smaller than this)
            ob = 0
            for i, grp_ in enumerate(groups):
                Ng = grp_[2].shape[-1]
                Kg = a.g[i].K
                ob += 4 * nb * (M * Kg + Ng * Kg + M * Ng * (2 if (a.flags & F_ACCUM) else 1))
            self._prof_end('gemm_%s_mfma_%s_%s' % ('bf16x3' if x3 else 'f32', variant, ('nt', 'nn', 'tn')[mode]), e0, flops, shape, ob)

    def slab_reduce(self, slabs, out, bias=None, flags=0):
        """slabs (S, rows, n) contiguous per slab; out (rows, n) view."""
        S, rows, n = slabs.shape
        assert slabs.stride(2) == 1 and slabs.stride(1) == n
        self._check(self.lib.dlsg_slab_reduce(_p(slabs), S, i64(slabs.stride(0)), _p(bias), _p(out), i64(rows), n,
                                              int(out.stride(0)), flags | (F_BIAS if bias is not None else 0),
                                              self._stream()), 'dlsg_slab_reduce')

    # ------------------------------------------------------------------ row kernels
    def _rowln_args(self, x, gamma, beta, y, stats, res, pe, pre_tanh, post_tanh, p1, site1, p2, site2, seed, eps):
        a = abi.dlsg_rowln_args()
        _chk2(x)
        a.x, a.ldx = _p(x), x.stride(0)
        a.res, a.ldres = _p(res), (res.stride(0) if res is not None else 0)
        a.gamma, a.beta = _p(gamma), _p(beta)
        a.y, a.ldy = _p(y), (y.stride(0) if y is not None else 0)
        a.stats = _p(stats)
        a.pe, a.pe_rows = _p(pe), (pe.size(0) if pe is not None else 1)
        a.rows, a.n = x.size(0), x.size(1)
        a.pre_tanh, a.post_tanh, a.eps = pre_tanh, post_tanh, eps
        a.p1, a.p2, a.site1, a.site2 = p1, p2, site1, site2
        a.seed, a.seed_ptr = _seed(seed)
        return a

    def rowln_fwd(self, x, gamma, beta, y, stats=None, res=None, pe=None, pre_tanh=0, post_tanh=0, p1=0.0, site1=0,
                  p2=0.0, site2=0, seed=0, eps=1e-5):
        a = self._rowln_args(x, gamma, beta, y, stats, res, pe, pre_tanh, post_tanh, p1, site1, p2, site2, seed, eps)
        self._check(self.lib.dlsg_rowln_fwd(C.byref(a), self._stream()), 'dlsg_rowln_fwd')

    def rowln_fwd_multi(self, items):
        """several norms of the same number of rows in ONE launch; items: dicts of rowln_fwd's arguments (x, gamma, beta, y, ...)"""
        n = len(items)
        if n == 1:
            return self.rowln_fwd(**items[0])
        arr = (abi.dlsg_rowln_args * n)()
        for i, it in enumerate(items):
            d = dict(stats=None, res=None, pe=None, pre_tanh=0, post_tanh=0, p1=0.0, site1=0, p2=0.0, site2=0, seed=0, eps=1e-5)
            d.update(it)
            arr[i] = self._rowln_args(d['x'], d['gamma'], d['beta'], d['y'], d['stats'], d['res'], d['pe'], d['pre_tanh'],
                                      d['post_tanh'], d['p1'], d['site1'], d['p2'], d['site2'], d['seed'], d['eps'])
        self._check(self.lib.dlsg_rowln_fwd_multi(arr, n, self._stream()), 'dlsg_rowln_fwd_multi')

    def rowln_bwd_multi(self, items):
        """several norm backwards of the same number of rows in ONE launch; items: dicts of rowln_bwd's arguments"""
        n = len(items)
        if n == 1:
            return self.rowln_bwd(**items[0])
        arr = (abi.dlsg_rowln_bwd_args * n)()
        for i, it in enumerate(items):
            d = dict(stats=None, res=None, pe=None, pre_tanh=0, post_tanh=0, p1=0.0, site1=0, p2=0.0, site2=0, seed=0, eps=1e-5,
                     dgb_part=None, accum_dx=False)
            d.update(it)
            b = arr[i]
            b.f = self._rowln_args(d['x'], d['gamma'], d['beta'], None, d['stats'], d['res'], d['pe'], d['pre_tanh'], d['post_tanh'],
                                   d['p1'], d['site1'], d['p2'], d['site2'], d['seed'], d['eps'])
            b.dy, b.lddy, b.dx, b.lddx = _p(d['dy']), d['dy'].stride(0), _p(d['dx']), d['dx'].stride(0)
            b.accum_dx = int(d['accum_dx'])
            b.dgb_part = _p(d['dgb_part'])
            b.nblk = d['dgb_part'].size(0) if d['dgb_part'] is not None else 0
        self._check(self.lib.dlsg_rowln_bwd_multi(arr, n, self._stream()), 'dlsg_rowln_bwd_multi')

    def rowln_bwd_nblk(self, rows):
        return self.lib.dlsg_rowln_bwd_nblk(int(rows))

    def rowln_bwd(self, dy, x, gamma, beta, dx, stats=None, res=None, pe=None, pre_tanh=0, post_tanh=0, p1=0.0,
                  site1=0, p2=0.0, site2=0, seed=0, eps=1e-5, dgb_part=None, accum_dx=False):
        b = abi.dlsg_rowln_bwd_args()
        b.f = self._rowln_args(x, gamma, beta, None, stats, res, pe, pre_tanh, post_tanh, p1, site1, p2, site2, seed,
                               eps)
        b.dy, b.lddy, b.dx, b.lddx = _p(dy), dy.stride(0), _p(dx), dx.stride(0)
        b.accum_dx = int(accum_dx)
        b.dgb_part = _p(dgb_part)
        b.nblk = dgb_part.size(0) if dgb_part is not None else 0
        self._check(self.lib.dlsg_rowln_bwd(C.byref(b), self._stream()), 'dlsg_rowln_bwd')

    def _colsum_ws(self, part):
        """scratch for the fixed-order combine of a tall input's row chunks (None: one chunk, nothing to combine)"""
        k = int(self.lib.dlsg_colsum_ws_floats(part.size(0), part.size(1)))
        return torch.empty(k, dtype=torch.float32, device=part.device) if k else None

    # Short column sums can be collected and launched together (`colsum_defer = []` starts collecting, `colsum_flush()` launches
    # and stops): the backward of a step folds ~25 small partial arrays, each 8-9 us on its own.
    colsum_defer = None

    def _colsum_try_defer(self, part, out_a, out_b, split, dup, accum):
        if self.colsum_defer is None or not self.lib.dlsg_colsum_multi_ok(_p(part), i64(part.stride(0)), part.size(0), part.size(1)):
            return False
        self.colsum_defer.append((part, out_a, out_b, split, dup, accum))
        return True

    def colsum_flush(self, keep_collecting=False):
        """launch the collected column sums: descriptors that write the same destination go into different launches, in order"""
        items, self.colsum_defer = (self.colsum_defer or []), ([] if keep_collecting else None)
        while items:
            batch, rest, seen = [], [], set()
            for it in items:
                dests = {it[1].data_ptr()} | ({it[2].data_ptr()} if it[2] is not None else set())
                if len(batch) < 32 and not (dests & seen) and not rest:
                    batch.append(it); seen |= dests
                else:
                    rest.append(it)
            arr = (abi.dlsg_colsum_desc * len(batch))()
            for d, (part, out_a, out_b, split, dup, accum) in zip(arr, batch):
                d.part, d.ld, d.out_a, d.out_b = _p(part), part.stride(0), _p(out_a), _p(out_b)
                d.rows, d.n, d.split, d.dup, d.accum = part.size(0), part.size(1), split, int(dup), int(accum)
            self._check(self.lib.dlsg_colsum_multi(arr, len(batch), self._stream()), 'dlsg_colsum_multi')
            items = rest

    def colsum(self, part, out, accum=False):
        """out[j] (+)= sum over rows of part (rows, n) view."""
        _chk2(part)
        if self._colsum_try_defer(part, out, None, part.size(1), False, accum):
            return
        ws = self._colsum_ws(part)
        self._check(self.lib.dlsg_colsum(_p(part), i64(part.stride(0)), part.size(0), part.size(1), _p(out), int(accum),
                                         _p(ws), self._stream()), 'dlsg_colsum')

    def colsum2(self, part, out_a, out_b, split=None, accum=False):
        """one pass, two destinations: split=k -> columns [0,k) to out_a and [k,n) to out_b; split=None -> every column
        to both out_a and out_b."""
        _chk2(part)
        if self._colsum_try_defer(part, out_a, out_b, 0 if split is None else split, split is None, accum):
            return
        ws = self._colsum_ws(part)
        self._check(self.lib.dlsg_colsum2(_p(part), i64(part.stride(0)), part.size(0), part.size(1), _p(out_a), _p(out_b),
                                          0 if split is None else split, int(split is None), int(accum), _p(ws), self._stream()),
                    'dlsg_colsum2')

    def softmax_fwd(self, x, y, outer, n, inner, mask=None):
        self._check(self.lib.dlsg_softmax_fwd(_p(x), _p(mask), _p(y), i64(outer), n, inner, self._stream()), 'softmax_fwd')

    def softmax_bwd(self, y, dy, dx, outer, n, inner):
        self._check(self.lib.dlsg_softmax_bwd(_p(y), _p(dy), _p(dx), i64(outer), n, inner, self._stream()), 'softmax_bwd')

    # ------------------------------------------------------------------ o2v graph
    def o2v_supported(self, T, H):
        return limits.o2v(T, H)

    def o2v_fwd(self, y, v, g_obj, b_obj, z, ml, ostats, S, scale, nsplit, eps=1e-5):
        self.o2v_fwd_multi([dict(y=y, v=v, g_obj=g_obj, b_obj=b_obj, z=z, ml=ml, ostats=ostats, S=S)], scale, nsplit, eps)

    def o2v_fwd_multi(self, items, scale, nsplit, eps=1e-5):
        """Several object->frame graphs of one shape in ONE launch (the object and the motion stream of CapGnnEncoder).
        items: dicts with y (B,NO,H), v (B,T,H), g_obj, b_obj, z, ml, ostats, S."""
        n = len(items)
        B, NO, H = items[0]['y'].shape
        T = items[0]['v'].shape[1]
        arr = (abi.dlsg_o2v_args * n)()
        wsb = self.lib.dlsg_o2v_workspace_bytes(B, T, H, nsplit)
        keep = []
        for a, it in zip(arr, items):
            assert it['y'].shape == (B, NO, H) and it['v'].shape[1] == T
            ws = torch.empty(wsb // 4, dtype=torch.float32, device=it['y'].device)
            keep.append(ws)
            a.y, a.v, a.g_obj, a.b_obj, a.z, a.ml, a.ostats, a.S = _p(it['y']), _p(it['v']), _p(it['g_obj']), _p(it['b_obj']), \
                _p(it['z']), _p(it['ml']), _p(it['ostats']), _p(it['S'])
            a.ws, a.ws_bytes = _p(ws), wsb
            a.B, a.T, a.NO, a.H, a.nsplit, a.scale, a.eps = B, T, NO, H, nsplit, scale, eps
        e0 = self._prof_begin()
        self._check(self.lib.dlsg_o2v_fwd_multi(arr, n, self._stream()), 'dlsg_o2v_fwd_multi')
        # algorithmic bytes: read y once + read v + write z, per graph
        self._prof_end('o2v_graph_fwd', e0, 4.0 * n * B * (NO * H + 2 * T * H), 'B=%d T=%d NO=%d H=%d streams=%d nsplit=%d' % (B, T, NO, H, n, nsplit))

    def o2v_bwd(self, y, ostats, g_obj, b_obj, v, z, dz, S, ml, dy, dv, scale, nsplit):
        """backward of o2v_fwd: dz (B,T,H) -> dy (B,NO,H), dv (B,T,H); returns part (B*nsplit,2,H) (obj_norm dgamma | dbeta per
        (clip, object chunk))."""
        return self.o2v_bwd_multi([dict(y=y, ostats=ostats, g_obj=g_obj, b_obj=b_obj, v=v, z=z, dz=dz, S=S, ml=ml, dy=dy, dv=dv)],
                                  scale, nsplit)[0]

    def o2v_bwd_multi(self, items, scale, nsplit):
        """the backward of several object->frame graphs of one shape, one launch per pass (both encoder streams).
        items: dicts with y (B,NO,H), ostats, g_obj, b_obj, v, z, dz (B,T,H), S, ml, dy, dv and optionally dysum (B*nsplit,H): the
        column sums of dy per (clip, object chunk).  Returns the list of `part` arrays."""
        n = len(items)
        B, NO, H = items[0]['y'].shape
        T = items[0]['v'].shape[1]
        dev = items[0]['y'].device
        arr = (abi.dlsg_o2v_bwd_args * n)()
        wsb = int(self.lib.dlsg_o2v_workspace_bytes(B, T, H, nsplit))
        keep, parts = [], []
        for a, it in zip(arr, items):
            for k in ('y', 'ostats', 'v', 'z', 'dz', 'S', 'ml', 'dy', 'dv'):
                _chkc(it[k])
            assert it['y'].shape == (B, NO, H) and it['v'].shape[1] == T
            pd = torch.empty(B, NO, 64, dtype=torch.float32, device=dev)
            m12 = torch.empty(B, NO, 2, dtype=torch.float32, device=dev)
            ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
            part = torch.empty(B * nsplit, 2, H, dtype=torch.float32, device=dev)
            keep += [pd, m12, ws]
            parts.append(part)
            for k in ('y', 'ostats', 'g_obj', 'b_obj', 'v', 'z', 'dz', 'S', 'ml', 'dy', 'dv'):
                setattr(a, k, _p(it[k]))
            a.pd, a.m12, a.part, a.ws, a.ws_bytes = _p(pd), _p(m12), _p(part), _p(ws), wsb
            if it.get('dysum') is not None:
                _chkc(it['dysum'])
                assert it['dysum'].shape == (B * nsplit, H)
                a.dysum = _p(it['dysum'])
            a.B, a.T, a.NO, a.H, a.nsplit, a.scale = B, T, NO, H, nsplit, scale
        e0 = self._prof_begin()
        self._check(self.lib.dlsg_o2v_bwd_multi(arr, n, self._stream()), 'dlsg_o2v_bwd_multi')
        # algorithmic bytes: y read by both passes is counted once (SURVEY.md 8d convention) + dy written + dz, v, dv
        self._prof_end('o2v_graph_bwd', e0, 4.0 * n * B * (2 * NO * H + 3 * T * H), 'B=%d T=%d NO=%d H=%d streams=%d nsplit=%d' % (B, T, NO, H, n, nsplit))
        return parts

    # ------------------------------------------------------------------ beam search
    @staticmethod
    def _beam_args(R, V, last, last_lp, pred, new_lp, back, rows, k, end, first, ended_count, logits=None):
        """dlsg_beam_select_args of one step on R = B*k rows; logits: the one model's (R, V) rows (an ensemble passes its own)"""
        a = abi.dlsg_beam_select_args()
        if logits is not None:
            a.logits, a.ld = _p(logits), logits.stride(0)
        a.last, a.last_lp = _p(last), _p(last_lp)
        a.pred, a.new_lp, a.back, a.rows, a.ended_count = _p(pred), _p(new_lp), _p(back), _p(rows), _p(ended_count)
        a.B, a.k, a.V, a.end, a.first = R // k, k, V, end, int(first)
        return a

    @staticmethod
    def _hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len, ended_count,
                   logits=None):
        """a history step at t (t == 0 is the first step) -> its dlsg_beam_select_args, and the arguments every history entry point
        takes alike: the two (R, L) history buffers, which are checked, L, t, no_repeat_ngram, min_len"""
        for h in (hist_in, hist_out):
            assert h.dtype == torch.int64 and h.is_contiguous() and h.shape == (R, hist_out.shape[1]), (h.dtype, h.shape)
        a = HipOps._beam_args(R, V, last, last_lp, pred, new_lp, back, rows, k, end, t == 0, ended_count, logits)
        return a, (_p(hist_in), _p(hist_out), hist_out.shape[1], int(t), int(no_repeat_ngram), int(min_len))

    @staticmethod
    def _beam_members(logits_list, weights, device):
        """checks the members' (R, V) logits -> R, V and the ctypes arguments (pointers, strides, weights normalised in float64,
        their logs, M) of dlsg_beam_select_ens / _groups"""
        M = len(logits_list)
        R, V = logits_list[0].shape
        for x in logits_list:
            assert x.dtype == torch.float32 and x.shape == (R, V) and x.stride(1) == 1 and x.device == device, (x.dtype, x.shape)
        assert len(weights) == M, (len(weights), M)
        w = normalised_weights(weights)
        return R, V, ((C.c_void_p * M)(*[x.data_ptr() for x in logits_list]), (C.c_int64 * M)(*[x.stride(0) for x in logits_list]),
                      (C.c_float * M)(*w), (C.c_float * M)(*[math.log(x) for x in w]), M)

    @staticmethod
    def _cons_dims(cons, d, B, device):
        """checks a constraint tensor of d dims on B clips, on the logits' device -> its dims behind the clips (None: no constraint)"""
        if cons is None:
            return (0,) + (1,) * (d - 2)
        assert cons.dtype == torch.int64 and cons.is_contiguous() and cons.dim() == d and cons.shape[0] == B, (cons.dtype, cons.shape)
        assert cons.device == device, (cons.device, device)
        return tuple(cons.shape[1:])

    @staticmethod
    def _chk_row_words(R, *outs):
        """checks the optional (R,) int32 outputs of a step"""
        for o in outs:
            if o is not None:
                assert o.dtype == torch.int32 and o.is_contiguous() and o.numel() == R, (o.dtype, o.shape)

    def beam_select(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, first=False, ended_count=None):
        """one beam-search step for every batch item (see include/dlsg.h): logits (B*k,V) -> pred/new_lp/back/rows (B*k)."""
        a = self._beam_args(*logits.shape, last, last_lp, pred, new_lp, back, rows, k, end, first, ended_count, logits)
        self._check(self.lib.dlsg_beam_select(C.byref(a), self._stream()), 'dlsg_beam_select')

    def beam_select_hist(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram=0,
                         min_len=0, ended_count=None):
        """`beam_select` at step t (t == 0 is the first step) with the beams' token history: hist_out[c] = hist_in[parent of c]
        with hist[t] = pred and `end` behind it ((B*k, L) int64, two buffers), a repeated-n-gram ban and a minimum length (see
        include/dlsg.h)."""
        a, hist = self._hist_step(*logits.shape, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram,
                                  min_len, ended_count, logits)
        self._check(self.lib.dlsg_beam_select_hist(C.byref(a), *hist, self._stream()), 'dlsg_beam_select_hist')

    def beam_select_cons(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, cons,
                         no_repeat_ngram=0, min_len=0, ended_count=None, met_out=None):
        """`beam_select_hist` for lexically constrained beam search: cons (B, C, W) int64 holds C sets of alternative word ids per
        clip (an id outside [0, V) is padding), a beam may end only once its history holds a word of every set, and the k new beams
        are allocated over the banks "number of constraints met", most first (see include/dlsg.h).  cons None, or C == 0: the bits
        of `beam_select_hist`.  met_out (B*k) int32, optional: the new beams' met masks."""
        R, V = logits.shape
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len,
                                  ended_count, logits)
        Cn, W = self._cons_dims(cons, 3, R // k, logits.device)
        self._chk_row_words(R, met_out)
        self._check(self.lib.dlsg_beam_select_cons(C.byref(a), *hist, _p(cons) if Cn else None, Cn, W, _p(met_out), self._stream()),
                    'dlsg_beam_select_cons')

    def beam_select_phrases(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, phr,
                            no_repeat_ngram=0, min_len=0, ended_count=None, met_out=None, bank_out=None):
        """`beam_select_cons` whose constraints are sets of alternative phrases: phr (B, C, W, P) int64 holds per clip C sets of W
        phrases of up to P <= 4 word ids (a phrase is the leading run of ids in [0, V)); a constraint is met once a phrase of its
        set stands in the beam's history as contiguous tokens, and the banks are (constraints met, progress into a phrase) (see
        include/dlsg.h).  P == 1: the bits of `beam_select_cons`; phr None, or C == 0: those of `beam_select_hist`.  met_out,
        bank_out (B*k) int32, optional: the new beams' met masks and banks."""
        R, V = logits.shape
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len,
                                  ended_count, logits)
        Cn, W, P = self._cons_dims(phr, 4, R // k, logits.device)
        self._chk_row_words(R, met_out, bank_out)
        self._check(self.lib.dlsg_beam_select_phrases(C.byref(a), *hist, _p(phr) if Cn else None, Cn, W, P, _p(met_out), _p(bank_out),
                                                      self._stream()), 'dlsg_beam_select_phrases')

    def beam_select_gumbel(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in, G_out,
                           temperature=1.0, seed=0, site_sample=0, no_repeat_ngram=0, min_len=0, ended_count=None):
        """`beam_select_hist` for stochastic beam search: the k new beams of a clip are the k largest perturbed values G (float64,
        (B*k), two buffers like last_lp / new_lp), rows in sampling order; last_lp / new_lp are log-probs under the tempered model
        renormalised over the unbanned words; the noise is `sample_embed`'s, keyed (seed, site_sample, ((t+1) R + r) V + j); seed an
        int or a device word (see include/dlsg.h)."""
        self._gumbel_step('dlsg_beam_select_gumbel', logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in,
                          G_out, temperature, seed, site_sample, no_repeat_ngram, min_len, ended_count)

    def _gumbel_step(self, entry, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in, G_out, temperature,
                     seed, site_sample, no_repeat_ngram, min_len, ended_count, tables=None):
        """the body of `beam_select_gumbel` and `beam_select_gumbel_excl`: `entry` with the (excl_shared, excl_clip) of `tables`
        behind its arguments"""
        R, V = logits.shape
        for G in (G_in, G_out):
            assert G.dtype == torch.float64 and G.is_contiguous() and G.numel() == R, (G.dtype, G.shape)
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len,
                                  ended_count, logits)
        tail = () if tables is None else self._excl_tables(*tables, R // k, logits.device)
        sd, sp = _seed(seed)
        self._check(getattr(self.lib, entry)(C.byref(a), *hist, f32(temperature), u64(sd), sp, u32(site_sample), _p(G_in), _p(G_out),
                                             *tail, self._stream()), entry)

    def beam_select_ens(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                        no_repeat_ngram=0, min_len=0, ended_count=None):
        """`beam_select_hist` for an ensemble: the candidates of beam row r are combined from logits_list[m][r], one (R, V) float32
        array per member, with `weights` (positive, normalised here in float64) -- mode 0: log of the weighted mean probability,
        mode 1: weighted mean log-probability (see include/dlsg.h)."""
        self._ens_step('dlsg_beam_select_ens', logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in,
                       hist_out, t, no_repeat_ngram, min_len, ended_count)

    def _ens_step(self, entry, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                  no_repeat_ngram, min_len, ended_count, tables=None):
        """the body of `beam_select_ens` and `beam_select_excl`: `entry` with the (excl_shared, excl_clip) of `tables` behind its
        arguments"""
        R, V, members = self._beam_members(logits_list, weights, hist_out.device)
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len,
                                  ended_count)
        tail = () if tables is None else self._excl_tables(*tables, R // k, hist_out.device)
        self._check(getattr(self.lib, entry)(C.byref(a), *members, int(mode), *hist, *tail, self._stream()), entry)

    def beam_select_groups(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                           no_repeat_ngram=0, min_len=0, num_groups=1, diversity_penalty=0.0, ended_count=None):
        """`beam_select_ens` for diverse beam search: the k beams of a clip are `num_groups` groups of consecutive rows, chosen one
        group after another; a word that earlier groups chose at this step from live beams costs a later group
        `diversity_penalty` per choice (inf: it is excluded).  new_lp stays the log-prob without the penalty (see include/dlsg.h).
        A single model passes one logits array and weights [1.0]."""
        R, V, members = self._beam_members(logits_list, weights, hist_out.device)
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, no_repeat_ngram, min_len,
                                  ended_count)
        self._check(self.lib.dlsg_beam_select_groups(C.byref(a), *members, int(mode), *hist, int(num_groups),
                                                     C.c_float(diversity_penalty), self._stream()), 'dlsg_beam_select_groups')

    @staticmethod
    def _excl_tables(shared, per_clip, B, device):
        """checks the two exclusion tables, (NS, P) shared and (B, NC, P) per clip, int64 on the logits' device, either None ->
        the ctypes arguments (shared, NS, per_clip, NC, P) of dlsg_beam_select_excl; an empty table goes as NULL with count 0"""
        P = None
        for tab, d, lim, what in ((shared, 2, abi.defines['DLSG_EXCL_SHARED'], 'shared'), (per_clip, 3, abi.defines['DLSG_EXCL_CLIP'], 'per-clip')):
            if tab is None:
                continue
            assert tab.dtype == torch.int64 and tab.is_contiguous() and tab.dim() == d, (what, tab.dtype, tab.shape)
            assert tab.device == device, (what, tab.device, device)
            assert d == 2 or tab.shape[0] == B, (what, tab.shape, B)
            assert tab.shape[-2] <= lim, (what, tab.shape, lim)
            if tab.shape[-2] > 0:
                assert 1 <= tab.shape[-1] <= abi.defines['DLSG_PHRASE_MAX'] and P in (None, tab.shape[-1]), (what, tab.shape, P)
                P = tab.shape[-1]
        NS = 0 if shared is None else shared.shape[0]
        NC = 0 if per_clip is None else per_clip.shape[1]
        return _p(shared) if NS else None, NS, _p(per_clip) if NC else None, NC, P or 1

    def beam_select_excl(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                         excl_shared=None, excl_clip=None, no_repeat_ngram=0, min_len=0, ended_count=None):
        """`beam_select_ens` with exclusions: excl_shared (NS <= 64, P) int64 holds entries of up to P <= 4 word ids that no clip's
        caption may contain, excl_clip (B, NC <= 32, P) each clip's own (an entry is the leading run of ids in [0, V)); a live beam
        may not choose the last word of an entry whose other words are the last words of its history (see include/dlsg.h).  Both
        None or empty: the bits of `beam_select_ens`.  A single model passes one logits array and weights [1.0]."""
        self._ens_step('dlsg_beam_select_excl', logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in,
                       hist_out, t, no_repeat_ngram, min_len, ended_count, (excl_shared, excl_clip))

    def beam_select_gumbel_excl(self, logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, G_in, G_out,
                                excl_shared=None, excl_clip=None, temperature=1.0, seed=0, site_sample=0, no_repeat_ngram=0, min_len=0,
                                ended_count=None):
        """`beam_select_gumbel` with the exclusion tables of `beam_select_excl`: the last words of the entries a live row's history
        leads up to join its ban list, and the log-probs are renormalised over the words that are left, as that step's other bans
        are (see include/dlsg.h).  Both tables None or empty: the bits of `beam_select_gumbel`."""
        self._gumbel_step('dlsg_beam_select_gumbel_excl', logits, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                          G_in, G_out, temperature, seed, site_sample, no_repeat_ngram, min_len, ended_count, (excl_shared, excl_clip))

    @staticmethod
    def _prefix_table(prefix, clips, device, what):
        """checks a prefix table, (clips, P) int64 on the logits' device -> P"""
        if not torch.is_tensor(prefix) or prefix.dtype != torch.int64 or prefix.dim() != 2 or not prefix.is_contiguous():
            raise ValueError('%s: prefix is a contiguous int64 tensor (B, P), not %s'
                             % (what, '%s %s' % (prefix.dtype, tuple(prefix.shape)) if torch.is_tensor(prefix) else type(prefix).__name__))
        if prefix.shape[0] != clips:
            raise ValueError('%s: the prefix of shape %s holds %d clips, the step %d' % (what, tuple(prefix.shape), prefix.shape[0], clips))
        if prefix.device != device:
            raise ValueError('%s: the prefix on %s, the logits on %s' % (what, prefix.device, device))
        return prefix.shape[1]

    def beam_force_prefix(self, logits_list, weights, mode, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t,
                          prefix):
        """A forced prefix behind a history step: called behind the step's select launch with that call's members and step
        arguments.  prefix (B, P) int64: a clip whose row holds ids in [0, V) at 0 .. t gets pred = prefix[b, t] in all its k slots,
        parent row b*k, that row's history with the word at t, new_lp = the parent's log-prob plus the word's value (`seq_logprob`'s
        bits) in slot 0 and -inf in the others; every other clip keeps what the select launch wrote (see include/dlsg.h).  A single
        model passes one logits array and weights [1.0]."""
        R, V, members = self._beam_members(logits_list, weights, hist_out.device)
        P = self._prefix_table(prefix, R // k, hist_out.device, 'beam_force_prefix')
        a, hist = self._hist_step(R, V, last, last_lp, pred, new_lp, back, rows, k, end, hist_in, hist_out, t, 0, 0, None)
        self._check(self.lib.dlsg_beam_force_prefix(C.byref(a), *members, int(mode), *hist[:4], _p(prefix) if P else None, P,
                                                    self._stream()), 'dlsg_beam_force_prefix')

    def beam_finalize(self, hist, lp, k, end, alpha, ids, scores, lens):
        """the n = ids.shape[1] best of each clip's k beams by lp / len^alpha: ids (B, n, L), scores (B, n), lens (B, n)."""
        R, L = hist.shape
        B, n = R // k, ids.shape[1]
        assert hist.dtype == torch.int64 and hist.is_contiguous() and lp.dtype == torch.float32 and lp.is_contiguous() and lp.numel() == R
        assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.shape == (B, n, L)
        assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (B, n)
        assert lens.dtype == torch.int64 and lens.is_contiguous() and lens.shape == (B, n)
        self._check(self.lib.dlsg_beam_finalize(_p(hist), _p(lp), B, k, L, i64(end), C.c_double(alpha), n, _p(ids), _p(scores), _p(lens),
                                                self._stream()), 'dlsg_beam_finalize')

    def seq_logprob(self, logits_list, weights, mode, ids, lens=None, length_penalty=0.0, want_tokens=False, want_ranks=False,
                    end=-1):
        """The log-probability of GIVEN captions (see include/dlsg.h, dlsg_seq_logprob): logits_list holds one float32 (L, R, V)
        view per member, row (t, r) what the member predicts for word t of caption r -- the decoder's time-major logits as they
        stand, an (R, L, V) tensor as `.transpose(0, 1)`; any time and row strides, unit stride along V.  weights, mode: as
        `beam_select_ens` takes them (one model: [1.0], 0).  ids (R, L) int64, rows any stride apart; lens (R) int64 or None: then
        a caption runs up to and including its first `end` (default -1: no such id, every caption is L words).  Returns (scores
        (R) float32 = lp / len^length_penalty, lens (R) int64, lp (R) float32, tok_lp (R, L) float32 or None, tok_rank (R, L) int32
        or None): only the rows of a caption's own words are read.  One launch; nothing is read back."""
        R, L = ids.shape
        dev = ids.device
        for x in logits_list:
            assert x.dim() == 3 and x.shape[0] >= L, (x.shape, L)
        _, V, members = self._beam_members([x[0] for x in logits_list], weights, dev)
        assert logits_list[0].shape[1] == R, (logits_list[0].shape, R)
        ld_t = (C.c_int64 * len(logits_list))(*[x.stride(0) for x in logits_list])
        assert ids.dtype == torch.int64 and (ids.stride(1) == 1 or L == 1) and (R <= 1 or ids.stride(0) >= L), (ids.dtype, ids.stride())
        if lens is not None:
            assert lens.dtype == torch.int64 and lens.is_contiguous() and lens.numel() == R and lens.device == dev, (lens.dtype, lens.shape)
        scores = torch.empty(R, dtype=torch.float32, device=dev)
        lens_out = torch.empty(R, dtype=torch.int64, device=dev)
        lp = torch.empty(R, dtype=torch.float32, device=dev)
        tok_lp = torch.empty(R, L, dtype=torch.float32, device=dev) if want_tokens else None
        tok_rank = torch.empty(R, L, dtype=torch.int32, device=dev) if want_ranks else None
        ptrs, ld_r, w, logw, M = members
        self._check(self.lib.dlsg_seq_logprob(ptrs, ld_t, ld_r, w, logw, M, int(mode), _p(ids), ids.stride(0) if R > 1 else L, _p(lens),
                                              R, L, V, i64(end), C.c_double(length_penalty), _p(tok_lp), _p(tok_rank), _p(lp),
                                              _p(scores), _p(lens_out), self._stream()), 'dlsg_seq_logprob')
        return scores, lens_out, lp, tok_lp, tok_rank

    def gather_rows_multi(self, srcs, rows, dsts):
        """dsts[i][r] = srcs[i][rows[r]] for up to 4 dense (R, n_i) arrays in one launch."""
        a = abi.dlsg_gather_multi_args()
        for i, (sr, ds) in enumerate(zip(srcs, dsts)):
            _chkc(sr); _chkc(ds)
            a.src[i], a.dst[i], a.n[i] = sr.data_ptr(), ds.data_ptr(), sr.shape[1]
        a.rows, a.nrows, a.count = _p(rows), rows.numel(), len(srcs)
        self._check(self.lib.dlsg_gather_rows_multi(C.byref(a), self._stream()), 'dlsg_gather_rows_multi')

    # ------------------------------------------------------------------ small per-clip graphs of the encoder
    def latent_psl_supported(self, T, P, H):
        return limits.latent_psl(T, P, H)

    def _psl_args(self, a, ov, theta, gamma, beta, adj, u, out, stats, p=0.0, site=0, seed=0, eps=1e-5):
        B, T, H = ov.shape
        P = theta.shape[0]
        for t in (ov, theta, adj, u, out, stats):
            _chkc(t)
        a.ov, a.theta, a.gamma, a.beta, a.adj, a.u, a.out, a.stats = _p(ov), _p(theta), _p(gamma), _p(beta), _p(adj), _p(u), \
            _p(out), _p(stats)
        a.B, a.T, a.P, a.H, a.p, a.site, a.eps = B, T, P, H, p, site, eps
        a.seed, a.seed_ptr = _seed(seed)

    def latent_psl_fwd(self, ov, theta, gamma, beta, adj, u, out, stats, p=0.0, site=0, seed=0, eps=1e-5):
        """ov (B,T,H), theta (P,H) -> adj (B,T,P), u (B*P,H) pre-activation, out (B*P,H), stats (B*P,2); one launch."""
        a = abi.dlsg_latent_psl_args()
        self._psl_args(a, ov, theta, gamma, beta, adj, u, out, stats, p, site, seed, eps)
        self._check(self.lib.dlsg_latent_psl_fwd(C.byref(a), self._stream()), 'dlsg_latent_psl_fwd')

    def latent_psl_fwd_multi(self, items):
        """several LatentPSL modules of one shape in ONE launch; items: dicts of latent_psl_fwd's arguments"""
        n = len(items)
        arr = (abi.dlsg_latent_psl_args * n)()
        for i, it in enumerate(items):
            self._psl_args(arr[i], **it)
        self._check(self.lib.dlsg_latent_psl_fwd_multi(arr, n, self._stream()), 'dlsg_latent_psl_fwd_multi')

    def latent_psl_bwd_supported(self, T, P, H):
        return limits.latent_psl_bwd(T, P, H)

    def _psl_bwd_args(self, a, dout, u, stats, gamma, adj, ov, theta, dov, dtheta_part, part, p=0.0, site=0, seed=0):
        B, T, H = ov.shape
        P = theta.shape[0]
        for t in (dout, u, stats, adj, ov, theta, dov, dtheta_part, part):
            _chkc(t)
        a.dout, a.u, a.stats, a.gamma, a.adj, a.ov, a.theta = _p(dout), _p(u), _p(stats), _p(gamma), _p(adj), _p(ov), _p(theta)
        a.dov, a.dtheta_part, a.part = _p(dov), _p(dtheta_part), _p(part)
        a.B, a.T, a.P, a.H, a.p, a.site = B, T, P, H, p, site
        a.seed, a.seed_ptr = _seed(seed)

    def latent_psl_bwd(self, dout, u, stats, gamma, adj, ov, theta, dov, dtheta_part, part, p=0.0, site=0, seed=0):
        """backward of latent_psl_fwd: dout (B*P,H) -> dov (B*T,H), dtheta_part (B,P,H), part (B,2,H); one launch."""
        a = abi.dlsg_latent_psl_bwd_args()
        self._psl_bwd_args(a, dout, u, stats, gamma, adj, ov, theta, dov, dtheta_part, part, p, site, seed)
        self._check(self.lib.dlsg_latent_psl_bwd(C.byref(a), self._stream()), 'dlsg_latent_psl_bwd')

    def latent_psl_bwd_multi(self, items):
        """several LatentPSL backwards of one shape in ONE launch; items: dicts of latent_psl_bwd's arguments"""
        n = len(items)
        arr = (abi.dlsg_latent_psl_bwd_args * n)()
        for i, it in enumerate(items):
            self._psl_bwd_args(arr[i], **it)
        self._check(self.lib.dlsg_latent_psl_bwd_multi(arr, n, self._stream()), 'dlsg_latent_psl_bwd_multi')

    def sa_core_supported(self, T, D):
        return limits.sa_core(T, D)

    def sa_core_fwd(self, K, Q, V, w, out, scale, mask=None):
        """K, Q, V (B,T,D) -> w (B,T,T) = softmax_j(K_i.Q_j*scale), out (B,T,D) = w V; one launch."""
        B, T, D = K.shape
        for t in (K, Q, V, w, out):
            _chkc(t)
        a = abi.dlsg_sa_core_args()
        a.K, a.Q, a.V, a.mask, a.w, a.out = _p(K), _p(Q), _p(V), _p(mask), _p(w), _p(out)
        a.B, a.T, a.D, a.scale = B, T, D, scale
        self._check(self.lib.dlsg_sa_core_fwd(C.byref(a), self._stream()), 'dlsg_sa_core_fwd')

    def sa_core_bwd(self, w, K, Q, V, dout, dK, dQ, dV, scale):
        """backward of sa_core_fwd: dout (B,T,D) + saved w (B,T,T) -> dK, dQ, dV (B,T,D); one launch."""
        B, T, D = K.shape
        for t in (w, K, Q, V, dout, dK, dQ, dV):
            _chkc(t)
        a = abi.dlsg_sa_core_bwd_args()
        a.w, a.K, a.Q, a.V, a.dout, a.dK, a.dQ, a.dV = _p(w), _p(K), _p(Q), _p(V), _p(dout), _p(dK), _p(dQ), _p(dV)
        a.B, a.T, a.D, a.scale = B, T, D, scale
        self._check(self.lib.dlsg_sa_core_bwd(C.byref(a), self._stream()), 'dlsg_sa_core_bwd')

    # ------------------------------------------------------------------ decoder attention
    def _decatt_args(self, Kp, Vp, q, c, alpha, scale):
        a = abi.dlsg_decatt_args()
        ns = len(Kp)
        B, P, Q = Kp[0].shape
        H = Vp[0].shape[2]
        for s in range(ns):
            a.Kp[s], a.Vp[s] = Kp[s].data_ptr(), Vp[s].data_ptr()
            if c is not None:
                a.c[s] = c[s].data_ptr()
        a.q, a.ldq = _p(q), q.stride(0)
        a.ldc = c[0].stride(0) if c is not None else 0
        a.alpha = _p(alpha)
        a.B, a.P, a.Q, a.H, a.nstream, a.scale = B, P, Q, H, ns, scale
        return a

    def decatt_fwd(self, Kp, Vp, q, c, alpha, scale):
        a = self._decatt_args(Kp, Vp, q, c, alpha, scale)
        self._check(self.lib.dlsg_decatt_fwd(C.byref(a), self._stream()), 'dlsg_decatt_fwd')

    def decatt_bwd(self, Kp, Vp, q, alpha, dc, dKp, dVp, dq, scale, accum_dq=False, dalpha=None):
        b = abi.dlsg_decatt_bwd_args()
        b.f = self._decatt_args(Kp, Vp, q, None, alpha, scale)
        for s in range(len(Kp)):
            b.dc[s], b.dKp[s], b.dVp[s] = dc[s].data_ptr(), dKp[s].data_ptr(), dVp[s].data_ptr()
        b.lddc = dc[0].stride(0)
        b.dalpha = _p(dalpha)
        b.dq, b.lddq, b.accum_dq = _p(dq), dq.stride(0), int(accum_dq)
        self._check(self.lib.dlsg_decatt_bwd(C.byref(b), self._stream()), 'dlsg_decatt_bwd')

    # ------------------------------------------------------------------ fused decoder step
    def dec_mid_fwd(self, slabs, addend, b_ih, b_hh, c_prev, c, h, gates, lnq, qcur, st_q, p_q, site_q, Kp, Vp, lnc, cpre,
                    ctx, st_c, alpha, p_att, site_att, scale, seed=0, eps=1e-5, kv_div=1, sched=0):
        """query cell pointwise -> LN(+dropout) -> attention over Kp/Vp (per stream) -> tanh -> LN(+dropout); one launch.
        lnq = (gamma, beta); lnc = [(gamma, beta)] per stream.  kv_div = k > 1: Kp / Vp hold one block per k consecutive rows
        (beam search: the k beams of a clip share their clip's K', V').  sched: 0 the library's choice, 1 loads where they are
        used, 2 loads requested up front (include/dlsg.h); the outputs are bit-identical."""
        a = abi.dlsg_dec_mid_args()
        a.kv_div, a.sched = kv_div, sched
        assert Kp[0].size(0) * max(1, kv_div) == c.size(0), (Kp[0].shape, c.shape, kv_div)
        a.slabs, a.nslab, a.slab_stride = _p(slabs), slabs.size(0), slabs.stride(0)
        a.addend, a.ldadd = _p(addend), (addend.stride(0) if addend is not None else 0)
        a.b_ih, a.b_hh, a.c_prev, a.c, a.h, a.gates = _p(b_ih), _p(b_hh), _p(c_prev), _p(c), _p(h), _p(gates)
        a.lnq_g, a.lnq_b, a.qcur, a.st_q, a.p_q, a.site_q = _p(lnq[0]), _p(lnq[1]), _p(qcur), _p(st_q), p_q, site_q
        ns = len(Kp)
        for i in range(ns):
            _chkc(Kp[i]); _chkc(Vp[i]); _chkc(cpre[i]); _chkc(ctx[i])
            a.Kp[i], a.Vp[i] = Kp[i].data_ptr(), Vp[i].data_ptr()
            a.lnc_g[i], a.lnc_b[i] = lnc[i][0].data_ptr(), lnc[i][1].data_ptr()
            a.cpre[i], a.ctx[i], a.st_c[i] = cpre[i].data_ptr(), ctx[i].data_ptr(), st_c[i].data_ptr()
            a.p_att[i], a.site_att[i] = p_att[i], site_att[i]
        for t in (c, h, gates, qcur, alpha):
            _chkc(t)
        a.alpha = _p(alpha)
        a.B, a.Q, a.H, a.P, a.nstream = c.size(0), c.size(1), Vp[0].size(2), Kp[0].size(1), ns
        a.scale, a.eps = scale, eps
        a.seed, a.seed_ptr = _seed(seed)
        self._check(self.lib.dlsg_dec_mid_fwd(C.byref(a), self._stream()), 'dlsg_dec_mid_fwd')

    # vocabulary x width up to which a workgroup projects its own row (dec_tail_fwd sample=).  The in-launch projection sums a row's
    # dot products in another order than the vocabulary GEMM whose logits the loss sees (and than the unfused path above this
    # size: MSR-VTT's 10 000 x 1024): two logits closer than ~1e-6 relative can order differently, so at an exact near-tie the
    # sampled word may differ from argmax(logits).  The reference itself is not bit-stable there (its GEMM's order is the
    # library's); every fixture with sampled steps -- reference-generated, both sides of this threshold -- gives identical ids
    # (tests/test_gpu_parity.py, test_gpu_bench_parity.py: MSVD below, MSR-VTT above).
    DEC_TAIL_SAMPLE_MAX_WEIGHTS = limits.DEC_TAIL_SAMPLE_MAX_WEIGHTS

    def dec_tail_sample_supported(self, V, D):
        return limits.dec_tail_sample(V, D)

    # s_split of every dec_tail_fwd(sample=...) launch: 0 the library's choice (dlsg_dec_tail_split), 1 unsplit, 2 ..
    # DLSG_DEC_TAIL_MAX_SPLIT forced (tests).  The outputs do not depend on it.
    dec_tail_split = 0

    def _dec_tail_ws(self, device, B):
        """the split scan's workspace of `device` (include/dlsg.h: zeroed once, here; every launch leaves it zeroed), one per
        device and kept.  Allocated and zeroed outside a capture only -- a step's warm-up launches come first -- so a capture
        that finds none large enough gets None, the unsplit launch."""
        ws = self._tail_ws.get(device)
        if ws is None or ws.numel() < B * abi.defines['DLSG_DEC_TAIL_WS_WORDS']:
            if torch.cuda.is_current_stream_capturing():
                return None
            ws = torch.zeros(max(B, 256) * abi.defines['DLSG_DEC_TAIL_WS_WORDS'], dtype=torch.int32, device=device)
            self._tail_ws[device] = ws
        return ws

    def dec_tail_fwd(self, slabs, b_ih, b_hh, c_prev, c, hd, gates, ln, dout, st_l, p, site, seed=0, eps=1e-5, sample=None):
        """language cell pointwise (+dropout on h) -> tanh(LN(h)); one launch.
        sample: optional dict(coins (int32 device vector), t, W (V,D), b (V) or None, E (V,Wd), ids_out (B) int64, we_out (B,Wd),
        p, site, row0): the next step's word is sampled inside the launch when coins[t] == 0 (include/dlsg.h); the vocabulary
        scan of such a step is split over the workgroups `dec_tail_split` says, on the workspace this object keeps."""
        a = abi.dlsg_dec_tail_args()
        if sample is not None:
            sm = sample
            for t_ in (sm['W'], sm['E'], sm['ids_out']):
                _chkc(t_)
            assert sm['W'].shape[1] == c.size(1) and sm['we_out'].stride(1) == 1 and sm['ids_out'].dtype == torch.int64
            a.s_coins, a.s_t, a.s_V = _p(sm['coins']), int(sm['t']), sm['W'].shape[0]
            a.s_W, a.s_b, a.s_E, a.s_Wd = _p(sm['W']), _p(sm.get('b')), _p(sm['E']), sm['E'].shape[1]
            a.s_site, a.s_ids, a.s_we, a.s_ldwe = sm.get('site', 0), _p(sm['ids_out']), _p(sm['we_out']), sm['we_out'].stride(0)
            a.s_row0, a.s_p = int(sm.get('row0', 0)), float(sm.get('p', 0.0))
            a.s_ws, a.s_split = _p(self._dec_tail_ws(c.device, c.size(0))), self.dec_tail_split
        a.slabs, a.nslab, a.slab_stride = _p(slabs), slabs.size(0), slabs.stride(0)
        a.b_ih, a.b_hh, a.c_prev, a.c, a.hd, a.gates = _p(b_ih), _p(b_hh), _p(c_prev), _p(c), _p(hd), _p(gates)
        for t in (c, hd, gates, dout):
            _chkc(t)
        a.ln_g, a.ln_b, a.dout, a.st_l, a.p, a.site = _p(ln[0]), _p(ln[1]), _p(dout), _p(st_l), p, site
        a.B, a.D, a.eps = c.size(0), c.size(1), eps
        a.seed, a.seed_ptr = _seed(seed)
        self._check(self.lib.dlsg_dec_tail_fwd(C.byref(a), self._stream()), 'dlsg_dec_tail_fwd')

    def dec_mid_bwd(self, slabs, dlh_rec, cpre, st_c, lnc_g, part_c, dcpre, p_att, site_att, Kp, Vp, alpha, dalpha, ds, qh,
                    st_q, lnq_g, part_q, p_q, site_q, rec_slabs, gates, c, c_prev, dc, dgates, scale, seed=0, sched=0):
        """backward of dec_mid_fwd for one word step (see include/dlsg.h).  slabs (S,B,ns*H+Q+D); dlh_rec (B,D) or None;
        rec_slabs (S',B,Q) view of the query cell's input-gradient slabs of step t+1, or None.  sched as in dec_mid_fwd."""
        a = abi.dlsg_dec_mid_bwd_args()
        a.sched = sched
        ns = len(Kp)
        B, Q = c.shape
        H, P = Vp[0].size(2), Kp[0].size(1)
        D = slabs.size(2) - ns * H - Q
        _chkc(slabs)
        a.slabs, a.nslab, a.slab_stride = _p(slabs), slabs.size(0), slabs.stride(0)
        a.write_rec, a.dlh_rec = int(dlh_rec is not None), _p(dlh_rec)
        for i in range(ns):
            for t in (cpre[i], part_c[i], dcpre[i], Kp[i], Vp[i]):
                _chkc(t)
            a.cpre[i], a.st_c[i], a.lnc_g[i] = cpre[i].data_ptr(), st_c[i].data_ptr(), lnc_g[i].data_ptr()
            a.part_c[i], a.dcpre[i] = part_c[i].data_ptr(), dcpre[i].data_ptr()
            a.p_att[i], a.site_att[i] = p_att[i], site_att[i]
            a.Kp[i], a.Vp[i] = Kp[i].data_ptr(), Vp[i].data_ptr()
        for t in (alpha, ds, qh, part_q, gates, c, dc, dgates) + ((dlh_rec,) if dlh_rec is not None else ()):
            _chkc(t)
        a.alpha, a.dalpha, a.ds = _p(alpha), _p(dalpha), _p(ds)
        a.qh, a.st_q, a.lnq_g, a.part_q, a.p_q, a.site_q = _p(qh), _p(st_q), _p(lnq_g), _p(part_q), p_q, site_q
        if rec_slabs is not None:
            a.rec_slabs, a.rec_nslab = _p(rec_slabs), rec_slabs.size(0)
            a.rec_slab_stride, a.rec_ld = rec_slabs.stride(0), rec_slabs.stride(1)
        a.gates, a.c, a.c_prev, a.dc, a.dgates = _p(gates), _p(c), _p(c_prev), _p(dc), _p(dgates)
        a.B, a.Q, a.H, a.D, a.P, a.nstream, a.scale = B, Q, H, D, P, ns, scale
        a.seed, a.seed_ptr = _seed(seed)
        self._check(self.lib.dlsg_dec_mid_bwd(C.byref(a), self._stream()), 'dlsg_dec_mid_bwd')

    def decatt_cache_grads(self, alpha, ds, qcur, dcpre, dKp, dVp):
        """dK'[s] = sum_t ds_t (x) q_cur_t, dV'[s] = sum_t alpha_t (x) dcpre_t  (time-major (L,B,.) inputs)."""
        a = abi.dlsg_decatt_cache_grads_args()
        L, B, Q = qcur.shape
        ns = len(dKp)
        for t in (alpha, ds, qcur):
            _chkc(t)
        a.alpha, a.ds, a.qcur = _p(alpha), _p(ds), _p(qcur)
        for i in range(ns):
            for t in (dcpre[i], dKp[i], dVp[i]):
                _chkc(t)
            a.dcpre[i], a.dKp[i], a.dVp[i] = dcpre[i].data_ptr(), dKp[i].data_ptr(), dVp[i].data_ptr()
        a.L, a.B, a.Q, a.H, a.P, a.nstream = L, B, Q, dVp[0].size(2), dKp[0].size(1), ns
        self._check(self.lib.dlsg_decatt_cache_grads(C.byref(a), self._stream()), 'dlsg_decatt_cache_grads')

    # ------------------------------------------------------------------ persistent kernels: time-out word
    def _persist_word(self, dev):
        """the int32 device word every persistent recurrent launch of this process reports a hand-off time-out into
        (csrc/bilstm.hip, csrc/critic_lstm.hip) and dlsg_adam reads as its guard"""
        w = getattr(self, '_persist_err', None)
        if w is None or w.device != dev:
            w = self._persist_err = torch.zeros(1, dtype=torch.int32, device=dev)
        return w

    guard_word = _persist_word        # (public name: the word a Trainer with several ranks max-reduces in front of Adam)

    def persist_word_or_none(self):
        """the time-out word (int32 device tensor) if a persistent kernel ran in this process: a caller that reads scalars back
        anyway appends it to that read and hands the value to `check_persistent(code=...)` -- one host synchronisation, not two"""
        return getattr(self, '_persist_err', None)

    def check_persistent(self, code=None):
        """Read the persistent kernels' time-out word: a workgroup that waited ~1 s for another one's flag (the launch was not
        fully co-resident: the device is shared with another process, or another stream held the compute units) sets it; results
        since then are invalid and every Adam launch since then was a no-op (dlsg_adam's guard).  Raises, after switching the
        BiLSTM to its step-by-step schedule for later launches.  A host synchronisation: called where a loss or token ids are read
        back anyway (Trainer.step every `check_every` steps, GanTrainer.iteration, beam.beam_finish, scoring.gather_results)."""
        w = getattr(self, '_persist_err', None)
        if w is None:
            return
        if code is None:
            code = int(w.item())
        if code:
            w.zero_()
            self.persistent_bilstm = False
            # graphs captured so far replay the persistent launches: their owners (Trainer, GanTrainer) compare this count and
            # capture again on the step-by-step schedule
            self.persist_timeouts = getattr(self, 'persist_timeouts', 0) + 1
            raise RuntimeError('persistent kernel hand-off timed out (code %d): the launch was not co-resident on this device.  '
                               'No parameter was updated by the steps since; the BiLSTM now runs step by step '
                               '(ops.persistent_bilstm = False)%s.  The critic\'s LSTM has no step-by-step form: GAN training needs '
                               'the device to itself.  Is the GPU shared with another process?' % (code, ''))

    # ------------------------------------------------------------------ persistent BiLSTM recurrence
    persistent_bilstm = True      # False: the per-step schedule (grouped skinny GEMM + pointwise launch per step)
    persistent_bilstm_bwd = True  # False: only the backward through time step by step (Trainer sets it when world_size > 1)

    def bilstm_supported(self, B, T, H):
        return self.persistent_bilstm and bool(self.lib.dlsg_bilstm_supported(B, T, H))

    def bilstm_fwd(self, xg, w_hh, b_ih, b_hh, out, hprev, c, gates):
        """all T steps of both directions in one launch (csrc/bilstm.hip).  xg[d] (B*T, 4H) rows b*T+t; out (B,T,2H);
        hprev[d] (B,T,H) zero-filled by the caller; c[d] (B,T,H); gates[d] (B,T,4H).  Returns the int32 error word (device)."""
        B, T, H2 = out.shape
        H = H2 // 2
        a = abi.dlsg_bilstm_args()
        dev = out.device
        hx = torch.empty(int(self.lib.dlsg_bilstm_hx_floats(T, H)), dtype=torch.float32, device=dev)
        flags = torch.empty(int(self.lib.dlsg_bilstm_flag_words(T, H)), dtype=torch.int32, device=dev)
        self._bilstm_err = self._persist_word(dev)
        for d in range(2):
            for t in (xg[d], w_hh[d], hprev[d], c[d], gates[d]):
                _chkc(t) if t is not xg[d] else _chk2(t)
            a.xg[d], a.w_hh[d], a.b_ih[d], a.b_hh[d] = xg[d].data_ptr(), w_hh[d].data_ptr(), b_ih[d].data_ptr(), b_hh[d].data_ptr()
            a.hprev[d], a.c[d], a.gates[d] = hprev[d].data_ptr(), c[d].data_ptr(), gates[d].data_ptr()
        _chkc(out)
        a.ldxg = xg[0].stride(0)
        assert xg[1].stride(0) == a.ldxg
        a.out, a.hx, a.flags, a.err = _p(out), _p(hx), _p(flags), _p(self._bilstm_err)
        a.B, a.T, a.H = B, T, H
        self._check(self.lib.dlsg_bilstm_fwd(C.byref(a), self._stream()), 'dlsg_bilstm_fwd')
        return self._bilstm_err

    def bilstm_bwd(self, gates, c, dout, w_hh, dgates):
        """backward through time of bilstm_fwd in one launch: dout (B,T,2H) -> dgates[d] (B,T,4H).  Returns the error word."""
        B, T, H2 = dout.shape
        H = H2 // 2
        a = abi.dlsg_bilstm_bwd_args()
        dev = dout.device
        nx = int(self.lib.dlsg_bilstm_bwd_x_floats(T, H))
        gx = torch.empty(nx, dtype=torch.float32, device=dev)
        px = torch.empty(nx, dtype=torch.float32, device=dev)
        flags = torch.empty(2 * int(self.lib.dlsg_bilstm_flag_words(T, H)), dtype=torch.int32, device=dev)
        self._bilstm_err = self._persist_word(dev)
        _chkc(dout)
        for d in range(2):
            for t in (gates[d], c[d], w_hh[d], dgates[d]):
                _chkc(t)
            a.gates[d], a.c[d], a.w_hh[d], a.dgates[d] = gates[d].data_ptr(), c[d].data_ptr(), w_hh[d].data_ptr(), dgates[d].data_ptr()
        a.dout, a.gx, a.px, a.flags, a.err = _p(dout), _p(gx), _p(px), _p(flags), _p(self._bilstm_err)
        a.B, a.T, a.H = B, T, H
        self._check(self.lib.dlsg_bilstm_bwd(C.byref(a), self._stream()), 'dlsg_bilstm_bwd')
        return self._bilstm_err

    # ------------------------------------------------------------------ critic LSTM, a whole sequence per launch
    def lstm_seq_supported(self, L, n, H):
        """the persistent launches take up to 256 sequences; more run as consecutive launches over caption chunks"""
        return bool(self.lib.dlsg_lstm_seq_supported(L, min(n, 256), H))

    def _lstm_seq(self, level, W, b_ih=None, b_hh=None, **t):
        """batch-major arrays (n, L, .): chunks of <= 256 sequences are independent recurrences, one persistent launch each"""
        ref = next(v for v in t.values() if v is not None)
        n, L = ref.shape[0], ref.shape[1]
        H = W.shape[1]
        dev = W.device
        # sequences per launch: as many row groups of 64 as the device can keep co-resident (256 rows need 4 x H / 8 workgroups
        # = 256 compute units at H = 512; a smaller part takes 192, 128 or 64 rows per launch)
        chunk = next((c for c in (256, 192, 128, 64) if self.lib.dlsg_lstm_seq_supported(L, min(n, c), H)), 0)
        if not chunk:
            raise RuntimeError('dlsg_lstm_seq does not take L = %d, H = %d on this device (H in {64, 512}, >= H / 8 compute units '
                               'per 64 sequences)' % (L, H))
        self._lstm_seq_err = self._persist_word(dev)
        _chkc(W)
        for name, v in t.items():
            if v is not None:
                _chkc(v)
                assert v.dtype == torch.float32 and v.shape[:2] == (n, L) and v.shape[2] in (H, 4 * H), (name, v.shape)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            a = abi.dlsg_lstm_seq_args()
            nx = int(self.lib.dlsg_lstm_seq_x_floats(L, hi - lo, H))
            xbuf = torch.empty(nx, dtype=torch.float32, device=dev)
            xbuf2 = torch.empty(nx, dtype=torch.float32, device=dev) if level == 1 else None
            flags = torch.empty(int(self.lib.dlsg_lstm_seq_flag_words(L, hi - lo, H)), dtype=torch.int32, device=dev)
            for name, v in t.items():
                setattr(a, name, _p(None if v is None else v[lo:hi]))
            a.W, a.xbuf, a.xbuf2, a.flags, a.err = _p(W), _p(xbuf), _p(xbuf2), _p(flags), _p(self._lstm_seq_err)
            a.b_ih, a.b_hh = _p(b_ih), _p(b_hh)
            a.L, a.n, a.H, a.batch_major = L, hi - lo, H, 1
            self._check(self.lib.dlsg_lstm_seq(C.byref(a), level, self._stream()), 'dlsg_lstm_seq(level %d)' % level)
        return self._lstm_seq_err

    def lstm_seq_fwd(self, xin, W, b_ih, b_hh, As, Hs, Cs, Hprev):
        """h_t, c_t for all L steps in one launch: xin (n, L, 4H) = x W_ih^T; W = weight_hh (4H, H); Hprev[:, t] = h_{t-1}."""
        return self._lstm_seq(0, W, b_ih, b_hh, addend=xin, As=As, Hs=Hs, Cs=Cs, Hprev=Hprev)

    def lstm_seq_bwd(self, As, Cs, W, dHs, dAs, dCs, DA, DH, DC):
        """backward through time with the injected gradients dAs / dCs (None = none) in one launch."""
        return self._lstm_seq(1, W, As=As, Cs=Cs, dHs=dHs, dAs=dAs, dCs=dCs, DA=DA, DH=DH, DC=DC)

    def lstm_seq_bwd2(self, As, Cs, W, DH, DC, ubar, gA, gC, gDH, gDHprev, gDC):
        """derivative of lstm_seq_bwd along ubar (n, L, 4H), the tangent of the input gates, in one launch"""
        return self._lstm_seq(2, W, As=As, Cs=Cs, DH=DH, DC=DC, addend=ubar, gA=gA, gC=gC, gDH=gDH, gDC=gDC, gDHprev=gDHprev)

    # ------------------------------------------------------------------ LSTM pointwise
    @staticmethod
    def _pw_fwd_args(a, slabs, c, B, H, addend=None, b_ih=None, b_hh=None, c_prev=None, h=None, h2=None, gates=None,
                     p=0.0, site=0, seed=0):
        if slabs is not None:
            a.slabs, a.nslab, a.slab_stride = _p(slabs), slabs.size(0), slabs.stride(0)
        else:
            a.slabs, a.nslab, a.slab_stride = None, 0, 0
        a.addend, a.ldadd = _p(addend), (addend.stride(0) if addend is not None else 0)
        a.b_ih, a.b_hh = _p(b_ih), _p(b_hh)
        a.c_prev, a.ldcp = _p(c_prev), (c_prev.stride(0) if c_prev is not None else 0)
        a.c, a.ldc_ = _p(c), c.stride(0)
        a.h, a.ldh = _p(h), (h.stride(0) if h is not None else 0)
        a.h2, a.ldh2 = _p(h2), (h2.stride(0) if h2 is not None else 0)
        a.gates, a.ldg = _p(gates), (gates.stride(0) if gates is not None else 0)
        a.B, a.H, a.p, a.site = B, H, p, site
        a.seed, a.seed_ptr = _seed(seed)

    def lstm_pw_fwd(self, slabs, c, B, H, **kw):
        a = abi.dlsg_lstm_pw_args()
        self._pw_fwd_args(a, slabs, c, B, H, **kw)
        self._check(self.lib.dlsg_lstm_pw_fwd(C.byref(a), self._stream()), 'dlsg_lstm_pw_fwd')

    def lstm_pw_fwd_multi(self, calls):
        """calls: 1 or 2 dicts of lstm_pw_fwd arguments (same B, H) -> one launch (both directions of a BiLSTM step)."""
        arr = (abi.dlsg_lstm_pw_args * len(calls))()
        for a, kw in zip(arr, calls):
            self._pw_fwd_args(a, **kw)
        self._check(self.lib.dlsg_lstm_pw_fwd_n(arr, len(calls), self._stream()), 'dlsg_lstm_pw_fwd_n')

    @staticmethod
    def _pw_bwd_args(a, gates, c, dgates, B, H, c_prev=None, dh=None, dh2=None, dc_next=None, dc_prev=None, p=0.0,
                     site=0, seed=0, dh3=None, dh4=None):
        a.gates, a.ldg, a.c, a.ldc_ = _p(gates), gates.stride(0), _p(c), c.stride(0)
        a.c_prev, a.ldcp = _p(c_prev), (c_prev.stride(0) if c_prev is not None else 0)
        a.dh, a.lddh = _p(dh), (dh.stride(0) if dh is not None else 0)
        a.dh2, a.lddh2 = _p(dh2), (dh2.stride(0) if dh2 is not None else 0)
        a.dh3, a.lddh3 = _p(dh3), (dh3.stride(0) if dh3 is not None else 0)
        if dh4 is not None and dh4.dim() == 3:      # slab stack (S,B,H): summed inside the kernel
            a.dh4, a.lddh4, a.dh4_nslab, a.dh4_slab_stride = _p(dh4), dh4.stride(1), dh4.size(0), dh4.stride(0)
        else:
            a.dh4, a.lddh4 = _p(dh4), (dh4.stride(0) if dh4 is not None else 0)
        a.dc_next, a.lddcn = _p(dc_next), (dc_next.stride(0) if dc_next is not None else 0)
        a.dgates, a.lddg = _p(dgates), dgates.stride(0)
        a.dc_prev, a.lddcp = _p(dc_prev), (dc_prev.stride(0) if dc_prev is not None else 0)
        a.B, a.H, a.p, a.site = B, H, p, site
        a.seed, a.seed_ptr = _seed(seed)

    def lstm_pw_bwd(self, gates, c, dgates, B, H, **kw):
        a = abi.dlsg_lstm_pw_bwd_args()
        self._pw_bwd_args(a, gates, c, dgates, B, H, **kw)
        self._check(self.lib.dlsg_lstm_pw_bwd(C.byref(a), self._stream()), 'dlsg_lstm_pw_bwd')

    def lstm_pw_bwd_multi(self, calls):
        arr = (abi.dlsg_lstm_pw_bwd_args * len(calls))()
        for a, kw in zip(arr, calls):
            self._pw_bwd_args(a, **kw)
        self._check(self.lib.dlsg_lstm_pw_bwd_n(arr, len(calls), self._stream()), 'dlsg_lstm_pw_bwd_n')

    # ------------------------------------------------------------------ movers
    def mean_rows_fwd(self, x, out):
        B, P, H = x.shape
        self._check(self.lib.dlsg_mean_rows_fwd(_p(x), _p(out), i64(out.stride(0)), B, P, H, self._stream()), 'mean_rows_fwd')

    def mean_rows_bwd(self, dout, dx, accum=False):
        B, P, H = dx.shape
        self._check(self.lib.dlsg_mean_rows_bwd(_p(dout), i64(dout.stride(0)), _p(dx), B, P, H, int(accum), self._stream()),
                    'mean_rows_bwd')

    def rows_repeat(self, x, y, n):
        """y[b*n + i] = x[b], i < n (x (B, ...) and y (B*n, ...) contiguous float32): x.repeat_interleave(n, 0) as one launch"""
        B = x.shape[0]
        assert x.is_contiguous() and y.is_contiguous() and y.shape[0] == B * n and y.shape[1:] == x.shape[1:], (x.shape, y.shape, n)
        self._check(self.lib.dlsg_rows_repeat(_p(x), _p(y), B, int(n), i64(x.numel() // max(B, 1)), self._stream()), 'rows_repeat')

    def clip_fold(self, dmem, dg, dx, n, accum=False):
        """dx[b,p,h] (+)= sum_{i<n} (dmem[b*n + i, p, h] + dg[b*n + i, h] / P); dg None, or (B*n, H) with any row stride"""
        B, P, H = dx.shape
        assert dmem.is_contiguous() and dx.is_contiguous() and dmem.shape == (B * n, P, H), (dmem.shape, dx.shape, n)
        assert dg is None or (dg.shape == (B * n, H) and dg.stride(1) == 1), (dg.shape, dg.stride())
        self._check(self.lib.dlsg_clip_fold(_p(dmem), _p(dg) if dg is not None else None, i64(dg.stride(0) if dg is not None else 0),
                                            _p(dx), B, int(n), P, H, int(accum), self._stream()), 'clip_fold')

    def embed_fwd(self, E, ids, out, p=0.0, seed=0, site=0, row0=0):
        rows, W = out.shape
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_embed_fwd(_p(E), _p(ids), _p(out), i64(out.stride(0)), rows, W, f32(p), u64(sd), u32(site),
                                            i64(row0), sp, self._stream()), 'embed_fwd')

    def select_embed(self, logits, captions, t, coins, E, ids_out, out, p=0.0, seed=0, site=0, row0=0, prefilled=False):
        """ids_out[b] = coins[t] ? captions[b, t] : argmax(logits[b]); out[b] = drop(E[id]).  prefilled: ids_out / out already
        hold the teacher-forced choice (the caller embedded every caption word in one launch): a no-op when coins[t] is set."""
        rows, V = logits.shape
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_select_embed(_p(logits), i64(logits.stride(0)), V, _p(captions), captions.shape[1], int(t),
                                               _p(coins), _p(E), _p(ids_out), _p(out), i64(out.stride(0)), rows, out.shape[1],
                                               f32(p), u64(sd), u32(site), i64(row0), sp, int(bool(prefilled)), self._stream()), 'select_embed')

    def embed_bwd(self, dout, ids, dE, p=0.0, seed=0, site=0, row0=0):
        rows, W = dout.shape
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_embed_bwd(_p(dout), i64(dout.stride(0)), _p(ids), _p(dE), rows, W, f32(p), u64(sd),
                                            u32(site), i64(row0), sp, self._stream()), 'embed_bwd')

    def argmax(self, logits, ids):
        rows, V = logits.shape
        self._check(self.lib.dlsg_argmax(_p(logits), i64(logits.stride(0)), _p(ids), rows, V, self._stream()), 'argmax')

    def _sample_args(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature, p, seed, site, site_sample, row0):
        """what `sample_embed` and `sample_filter_embed` ask of their common arguments, and the arguments their entry points
        share (everything in front of the filter's controls)"""
        rows, V = logits.shape
        assert E.shape[0] >= V and E.is_contiguous() and ids_out.numel() == rows and logp.numel() == rows and lens.numel() == rows
        assert ids_out.dtype == torch.int64 and lens.dtype == torch.int64 and out.shape == (rows, E.shape[1])
        sd, sp = _seed(seed)
        vp = C.c_void_p                                     # (none of the six is None)
        return (vp(logits.data_ptr()), i64(logits.stride(0)), V, f32(temperature), vp(E.data_ptr()), vp(ids_out.data_ptr()),
                vp(out.data_ptr()), i64(out.stride(0)), out.shape[1], vp(logp.data_ptr()), vp(lens.data_ptr()), int(t), i64(end_id),
                rows, f32(p), u64(sd), u32(site), u32(site_sample), i64(row0), sp)

    def sample_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0, site_sample=0,
                     row0=0):
        """ids_out[r] ~ softmax(logits[r] / temperature) (Gumbel-max on the (seed, site_sample, row0 + r) noise; 0: argmax),
        logp[r] = its log-probability, out[r] = drop(E[id]) on the word-dropout rows row0 + r, lens[r] = t + 1 at the first end_id
        (the caller sets lens to L)."""
        args = self._sample_args(logits, E, ids_out, out, logp, lens, t, end_id, temperature, p, seed, site, site_sample, row0)
        self._check(self.lib.dlsg_sample_embed(*args, self._stream()), 'sample_embed')

    def sample_filter_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0, site_sample=0,
                            row0=0, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None):
        """`sample_embed` on the truncated distribution: <end> banned while t < min_len, the classes that would repeat a
        no_repeat_ngram-gram of the row's history banned (hist: (>= t, rows) int64 time-major, the rows' earlier words), then
        top_k and top_p; the noise of a word is `sample_embed`'s.  logp is the log-probability under the truncated
        distribution, kept (rows,) int32 or None the number of words kept (include/dlsg.h)."""
        rows, V = logits.shape
        if V > SAMPLE_FILTER_MAXV:
            raise ValueError('sample_filter_embed holds a row of logits in LDS: vocabulary %d > %d' % (V, SAMPLE_FILTER_MAXV))
        args = self._sample_args(logits, E, ids_out, out, logp, lens, t, end_id, temperature, p, seed, site, site_sample, row0)
        assert kept is None or (kept.dtype == torch.int32 and kept.numel() == rows and kept.is_contiguous())
        if no_repeat_ngram > 0 and t > 0:
            assert hist is not None and hist.dtype == torch.int64 and hist.shape[0] >= t and hist.shape[1] == rows and \
                hist.stride(1) == 1, 'hist: the rows\' earlier words, (>= t, rows) int64'
        self._check(self.lib.dlsg_sample_filter_embed(
            *args, int(top_k), f32(top_p), int(min_len), int(no_repeat_ngram), _p(hist) if hist is not None else None,
            i64(hist.stride(0) if hist is not None else 0), _p(kept) if kept is not None else None, self._stream()),
            'sample_filter_embed')

    def sample_excl_embed(self, logits, E, ids_out, out, logp, lens, t, end_id, temperature=1.0, p=0.0, seed=0, site=0, site_sample=0,
                          row0=0, top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None, excl_shared=None,
                          excl_clip=None, rows_per_clip=1):
        """`sample_filter_embed` under the exclusion tables of `beam_select_excl`: excl_shared (NS <= 64, P) int64 for every row,
        excl_clip (rows / rows_per_clip, NC <= 32, P) of which row r reads clip r // rows_per_clip's; the last word of an entry is
        banned behind its other words, before top_k and top_p, and logp is renormalised over the words that are left (see
        include/dlsg.h).  hist as there, needed from t = 1 on with an entry.  Both tables None or empty: the bits of
        `sample_filter_embed`."""
        rows, V = logits.shape
        if V > SAMPLE_FILTER_MAXV:
            raise ValueError('sample_excl_embed holds a row of logits in LDS: vocabulary %d > %d' % (V, SAMPLE_FILTER_MAXV))
        if rows_per_clip < 1 or rows % rows_per_clip:
            raise ValueError('sample_excl_embed: %d rows are not clips of rows_per_clip = %r rows' % (rows, rows_per_clip))
        args = self._sample_args(logits, E, ids_out, out, logp, lens, t, end_id, temperature, p, seed, site, site_sample, row0)
        assert kept is None or (kept.dtype == torch.int32 and kept.numel() == rows and kept.is_contiguous())
        tables = self._excl_tables(excl_shared, excl_clip, rows // rows_per_clip, logits.device)
        if (no_repeat_ngram > 0 or tables[1] + tables[3] > 0) and t > 0:
            assert hist is not None and hist.dtype == torch.int64 and hist.shape[0] >= t and hist.shape[1] == rows and \
                hist.stride(1) == 1, 'hist: the rows\' earlier words, (>= t, rows) int64'
        self._check(self.lib.dlsg_sample_excl_embed(
            *args, int(top_k), f32(top_p), int(min_len), int(no_repeat_ngram), _p(hist) if hist is not None else None,
            i64(hist.stride(0) if hist is not None else 0), _p(kept) if kept is not None else None, *tables, int(rows_per_clip),
            self._stream()), 'sample_excl_embed')

    def sample_ens(self, logits_list, weights, mode, comb, ids_out, logp, lens, t, end_id, temperature=1.0, seed=0, site_sample=0, row0=0,
                   top_k=0, top_p=1.0, min_len=0, no_repeat_ngram=0, hist=None, kept=None, excl_shared=None, excl_clip=None,
                   rows_per_clip=1):
        """A sampled word step of an ensemble: logits_list, weights, mode as `beam_select_ens` takes them; comb (rows, V) float32,
        contiguous: the caller's workspace, which holds the rows' combined values on return; then ids_out[r] drawn from
        exp(comb[r] / temperature) under the controls and tables of `sample_excl_embed`, with that step's noise, logp, lens and kept --
        the bits of that step on comb as its logits -- and no embedding: the members embed the word themselves (see
        include/dlsg_sample_ens.h)."""
        rows, V, members = self._beam_members(logits_list, weights, comb.device)
        control = top_k > 0 or top_p < 1.0 or min_len > 0 or no_repeat_ngram > 0
        tables = self._excl_tables(excl_shared, excl_clip, rows // rows_per_clip if rows_per_clip >= 1 else 0, comb.device)
        if V > SAMPLE_FILTER_MAXV and (control or tables[1] + tables[3] > 0):
            raise ValueError('sample_ens holds a row of combined values in LDS under a control: vocabulary %d > %d' % (V, SAMPLE_FILTER_MAXV))
        if rows_per_clip < 1 or rows % rows_per_clip:
            raise ValueError('sample_ens: %d rows are not clips of rows_per_clip = %r rows' % (rows, rows_per_clip))
        assert comb.dtype == torch.float32 and comb.shape == (rows, V) and comb.is_contiguous(), (comb.dtype, comb.shape)
        assert ids_out.numel() == rows and logp.numel() == rows and lens.numel() == rows
        assert ids_out.dtype == torch.int64 and lens.dtype == torch.int64 and logp.dtype == torch.float32
        assert kept is None or (kept.dtype == torch.int32 and kept.numel() == rows and kept.is_contiguous())
        if (no_repeat_ngram > 0 or tables[1] + tables[3] > 0) and t > 0:
            assert hist is not None and hist.dtype == torch.int64 and hist.shape[0] >= t and hist.shape[1] == rows and \
                hist.stride(1) == 1, 'hist: the rows\' earlier words, (>= t, rows) int64'
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_sample_ens(
            *members, int(mode), V, f32(temperature), _p(comb), _p(ids_out), _p(logp), _p(lens), int(t), i64(end_id), rows, u64(sd),
            u32(site_sample), i64(row0), sp, int(top_k), f32(top_p), int(min_len), int(no_repeat_ngram),
            _p(hist) if hist is not None else None, i64(hist.stride(0) if hist is not None else 0), _p(kept), *tables,
            int(rows_per_clip), self._stream()), 'sample_ens')

    def sample_force_prefix(self, logits, E, ids_out, out, logp, lens, t, prefix, L, temperature=1.0, p=0.0, seed=0, site=0, row0=0,
                            rows_per_clip=1, kept=None):
        """A forced prefix behind a sampled step: called behind `sample_embed`, `sample_filter_embed` or `sample_excl_embed` with
        that call's logits, E, ids_out, out, logp, lens, t, temperature, p, seed, site and row0.  prefix (rows / rows_per_clip, P)
        int64, of which row r reads clip r // rows_per_clip's: a row whose clip holds ids in [0, V) at 0 .. t gets ids_out =
        prefix[., t], logp = that word's plain log-probability under softmax(logits / temperature) -- `sample_embed`'s bits for a
        word it draws --, out = drop(E[word]), lens = L and kept = 1; every other row keeps what the step wrote (see
        include/dlsg.h)."""
        rows, V = logits.shape
        if rows_per_clip < 1 or rows % rows_per_clip:
            raise ValueError('sample_force_prefix: %d rows are not clips of rows_per_clip = %r rows' % (rows, rows_per_clip))
        P = self._prefix_table(prefix, rows // rows_per_clip, logits.device, 'sample_force_prefix')
        assert logits.dtype == torch.float32 and logits.stride(1) == 1 and logp.dtype == torch.float32, (logits.dtype, logits.stride())
        assert E.shape[0] >= V and E.is_contiguous() and ids_out.numel() == rows and logp.numel() == rows and lens.numel() == rows
        assert ids_out.dtype == torch.int64 and lens.dtype == torch.int64 and out.shape == (rows, E.shape[1])
        assert kept is None or (kept.dtype == torch.int32 and kept.numel() == rows and kept.is_contiguous())
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_sample_force_prefix(
            _p(logits), i64(logits.stride(0)), V, f32(temperature), _p(E), _p(ids_out), _p(out), i64(out.stride(0)), out.shape[1],
            _p(logp), _p(lens), int(t), rows, f32(p), u64(sd), u32(site), i64(row0), sp, _p(prefix) if P else None, P,
            int(rows_per_clip), int(L), _p(kept), self._stream()), 'sample_force_prefix')

    def copy2d(self, src, dst, accum=False):
        rows, n = src.shape
        self._check(self.lib.dlsg_copy2d(_p(src), i64(src.stride(0)), _p(dst), i64(dst.stride(0)), rows, n, int(accum),
                                         self._stream()), 'copy2d')

    def dropout(self, x, y, p, seed, site):
        rows, n = x.shape
        sd, sp = _seed(seed)
        self._check(self.lib.dlsg_dropout(_p(x), i64(x.stride(0)), _p(y), i64(y.stride(0)), rows, n, f32(p), u64(sd),
                                          u32(site), sp, self._stream()), 'dropout')

    def fill(self, t, value):
        assert t.is_contiguous()
        self._check(self.lib.dlsg_fill(_p(t), i64(t.numel()), f32(value), self._stream()), 'fill')

    # ------------------------------------------------------------------ critic schedule blocks (csrc/critic_sched.hip)
    def crit_embed_mix(self, proj_tm, ids, W, bias, eps, h):
        ng, B, L, _ = h.shape
        self._check(self.lib.dlsg_crit_embed_mix(_p(proj_tm), _p(ids), _p(W), _p(bias), _p(eps), _p(h), ng, B, L, W.shape[1],
                                                 self._stream()), 'crit_embed_mix')

    def crit_embed_mix_bwd(self, ch, eps, dhr, dhf_tm):
        ng, B, L, _ = ch.shape
        self._check(self.lib.dlsg_crit_embed_mix_bwd(_p(ch), _p(eps), _p(dhr), _p(dhf_tm), ng, B, L, self._stream()), 'crit_embed_mix_bwd')

    def crit_vocab_scatter(self, dhr, ids, dW):
        _chkc(dhr); _chkc(ids); _chkc(dW)
        self._check(self.lib.dlsg_crit_vocab_scatter(_p(dhr), _p(ids), _p(dW), ids.numel(), dW.shape[1], self._stream()), 'crit_vocab_scatter')

    def crit_relu_taps(self, x, ref, bias, bias_scale, y, taps):
        n, L, _ = x.shape
        for t in (x, ref, y, taps):
            _chkc(t)
        self._check(self.lib.dlsg_crit_relu_taps(_p(x), _p(ref), _p(bias), f32(bias_scale), _p(y), _p(taps), n, L, self._stream()),
                    'crit_relu_taps')

    def crit_relu_taps_bwd(self, dy, dtaps, ref, dx):
        n, L, _ = dy.shape
        for t in (dy, dtaps, ref, dx):
            _chkc(t)
        self._check(self.lib.dlsg_crit_relu_taps_bwd(_p(dy), _p(dtaps), _p(ref), _p(dx), n, L, self._stream()), 'crit_relu_taps_bwd')

    def _cln_args(self, x, gamma, pre_tanh, eps, p_pre, site_pre, p_post, site_post, seed, row0):
        a = abi.dlsg_cln_args()
        G = len(x)
        rows, N = x[0].shape
        for g in range(G):
            _chkc(x[g]); _chkc(gamma[g])
            assert x[g].shape == (rows, N) and x[g].dtype == torch.float32
            a.x[g], a.gamma[g] = _p(x[g]), _p(gamma[g])
        a.rows, a.N, a.groups, a.pre_tanh, a.eps = rows, N, G, int(pre_tanh), eps
        a.p_pre, a.site_pre, a.p_post, a.site_post, a.row0 = p_pre, site_pre, p_post, site_post, row0
        a.seed, a.seed_ptr = _seed(seed)
        a.acc_lo = a.acc_hi = 0
        return a

    def _cln_ws(self, a, dev):
        return torch.empty(a.groups * int(self.lib.dlsg_cln_ws_floats(a.rows, a.N)), dtype=torch.float32, device=dev)

    @staticmethod
    def _cln_dys(a, dys):
        a.ndy = len(dys)
        for k, lst in enumerate(dys):
            for g, t in enumerate(lst):
                _chkc(t)
                a.dy[k][g] = _p(t)

    def cln_fwd(self, x, gamma, beta, y, pre_tanh, eps=1e-5, p_pre=0.0, site_pre=0, p_post=0.0, site_post=0, seed=0, row0=0):
        a = self._cln_args(x, gamma, pre_tanh, eps, p_pre, site_pre, p_post, site_post, seed, row0)
        for g in range(len(x)):
            _chkc(y[g])
            a.beta[g], a.y[g] = _p(beta[g]), _p(y[g])
        self._check(self.lib.dlsg_cln_fwd(C.byref(a), self._stream()), 'cln_fwd')

    def cln_ws_rows(self, rows, N):
        """rows of the per-workgroup partial arrays cln_bwd / cln_bwd2 leave in a deferred workspace (G, 2, this, N)"""
        return int(self.lib.dlsg_cln_ws_floats(rows, N)) // (2 * N)

    def cln_bwd(self, x, gamma, dys, dx, dgamma, dbeta, pre_tanh, eps=1e-5, p_pre=0.0, site_pre=0, p_post=0.0, site_post=0, seed=0,
                row0=0, acc=None, extra=None, defer_ws=None):
        """defer_ws (G, 2, cln_ws_rows, N): the per-workgroup partials of (dgamma, dbeta) are left there, unfolded (the caller sums the
        rows); dgamma / dbeta / extra are then ignored"""
        a = self._cln_args(x, gamma, pre_tanh, eps, p_pre, site_pre, p_post, site_post, seed, row0)
        self._cln_dys(a, dys)
        for g in range(len(x)):
            _chkc(dx[g])
            a.dx[g] = _p(dx[g])
            if dgamma and defer_ws is None:
                a.dgamma[g], a.dbeta[g] = _p(dgamma[g]), _p(dbeta[g])
                if extra is not None:
                    _chkc(extra[g])
                    a.extra[g] = _p(extra[g])
        if acc is not None:
            a.acc_lo, a.acc_hi = acc
        if defer_ws is not None:
            _chkc(defer_ws)
            assert tuple(defer_ws.shape) == (len(x), 2, self.cln_ws_rows(a.rows, a.N), a.N), defer_ws.shape
            ws, a.defer = defer_ws, 1
        else:
            ws = self._cln_ws(a, x[0].device) if dgamma else None
        a.ws = _p(ws)
        self._check(self.lib.dlsg_cln_bwd(C.byref(a), self._stream()), 'cln_bwd')

    def cln_bwd2(self, x, gamma, dys, U, gx, gdy, gpart, pre_tanh, eps=1e-5, p_pre=0.0, site_pre=0, p_post=0.0, site_post=0, seed=0,
                 row0=0, defer_ws=None):
        a = self._cln_args(x, gamma, pre_tanh, eps, p_pre, site_pre, p_post, site_post, seed, row0)
        self._cln_dys(a, dys)
        for g in range(len(x)):
            for t in (U[g], gx[g], gdy[g]):
                _chkc(t)
            a.U[g], a.gx[g], a.gdy[g] = _p(U[g]), _p(gx[g]), _p(gdy[g])
            if defer_ws is None:
                _chkc(gpart[g])
                a.gpart[g] = _p(gpart[g])
        if defer_ws is not None:
            _chkc(defer_ws)
            assert tuple(defer_ws.shape) == (len(x), 2, self.cln_ws_rows(a.rows, a.N), a.N), defer_ws.shape
            ws, a.defer = defer_ws, 1
        else:
            ws = self._cln_ws(a, x[0].device)
        a.ws = _p(ws)
        self._check(self.lib.dlsg_cln_bwd2(C.byref(a), self._stream()), 'cln_bwd2')

    def _sa_args(self, KQV, smask, scale, acc=None):
        a = abi.dlsg_crit_sa_args()
        _chkc(KQV); _chkc(smask)
        a.KQV, a.smask = _p(KQV), _p(smask)
        a.n, a.L, a.B, a.scale = KQV.shape[0], KQV.shape[1], smask.shape[0], scale
        a.acc_lo, a.acc_hi = acc if acc is not None else (0, 0)
        return a

    def crit_sa_fwd(self, KQV, smask, w, ctx, scale):
        a = self._sa_args(KQV, smask, scale)
        _chkc(w); _chkc(ctx)
        a.w, a.ctx = _p(w), _p(ctx)
        self._check(self.lib.dlsg_crit_sa_fwd(C.byref(a), self._stream()), 'crit_sa_fwd')

    def crit_sa_bwd(self, KQV, smask, w, dctx, dKQV, scale, acc=None):
        a = self._sa_args(KQV, smask, scale, acc)
        for t in (w, dctx, dKQV):
            _chkc(t)
        a.w, a.dctx, a.dKQV = _p(w), _p(dctx), _p(dKQV)
        self._check(self.lib.dlsg_crit_sa_bwd(C.byref(a), self._stream()), 'crit_sa_bwd')

    def crit_sa_bwd2(self, KQV, smask, w, dctx, U, Uctx, gKQV, scale):
        a = self._sa_args(KQV, smask, scale)
        for t in (w, dctx, U, Uctx, gKQV):
            _chkc(t)
        a.w, a.dctx, a.U, a.Uctx, a.gKQV = _p(w), _p(dctx), _p(U), _p(Uctx), _p(gKQV)
        self._check(self.lib.dlsg_crit_sa_bwd2(C.byref(a), self._stream()), 'crit_sa_bwd2')

    @staticmethod
    def _set2(st_, **kw):
        for name, pair in kw.items():
            if pair is None:
                continue
            arr = getattr(st_, name)
            for h in range(2):
                _chkc(pair[h])
                arr[h] = _p(pair[h])

    def _pattn_args(self, a_, e, smask, scale, acc=None):
        a = abi.dlsg_crit_pattn_args()
        self._set2(a, a=a_, e=e)
        _chkc(smask)
        a.smask = _p(smask)
        a.n, a.L, a.B, a.T, a.scale = a_[0].shape[0], a_[0].shape[1], smask.shape[0], e[0].shape[1], scale
        a.acc_lo, a.acc_hi = acc if acc is not None else (0, 0)
        return a

    def crit_pattn_fwd(self, a_, e, smask, P, wgt, aggpre, scale):
        a = self._pattn_args(a_, e, smask, scale)
        self._set2(a, P=P, wgt=wgt, aggpre=aggpre)
        self._check(self.lib.dlsg_crit_pattn_fwd(C.byref(a), self._stream()), 'crit_pattn_fwd')

    def crit_pattn_bwd(self, a_, e, smask, P, d_agg, d_wgt, da, de, scale, acc=None):
        a = self._pattn_args(a_, e, smask, scale, acc)
        self._set2(a, P=P, d_agg=d_agg, d_wgt=d_wgt, da=da, de=de)
        self._check(self.lib.dlsg_crit_pattn_bwd(C.byref(a), self._stream()), 'crit_pattn_bwd')

    def crit_pattn_bwd2(self, a_, e, smask, P, d_agg, d_wgt, Ua, Uagg, Uwgt, ga, ge, scale):
        a = self._pattn_args(a_, e, smask, scale)
        self._set2(a, P=P, d_agg=d_agg, d_wgt=d_wgt, Ua=Ua, Uagg=Uagg, Uwgt=Uwgt, ga=ga, ge=ge)
        self._check(self.lib.dlsg_crit_pattn_bwd2(C.byref(a), self._stream()), 'crit_pattn_bwd2')

    def _tsum_args(self, words, theta, gamma, beta, fusion, eps, p, site, seed, row0, acc=None):
        a = abi.dlsg_crit_tsum_args()
        for t in (words, theta, gamma, fusion):
            _chkc(t)
        a.words, a.theta, a.gamma, a.beta, a.fusion = _p(words), _p(theta), _p(gamma), _p(beta), _p(fusion)
        a.n, a.L, a.eps, a.p, a.site, a.row0 = words.shape[0], words.shape[1], eps, p, site, row0
        a.seed, a.seed_ptr = _seed(seed)
        a.acc_lo, a.acc_hi = acc if acc is not None else (0, 0)
        return a

    def crit_tsum_fwd(self, words, theta, gamma, beta, fusion, adj, u, sent, fus, eps=1e-5, p=0.0, site=0, seed=0, row0=0):
        a = self._tsum_args(words, theta, gamma, beta, fusion, eps, p, site, seed, row0)
        for t in (adj, u, sent, fus):
            _chkc(t)
        a.adj, a.u, a.sent, a.fus = _p(adj), _p(u), _p(sent), _p(fus)
        self._check(self.lib.dlsg_crit_tsum_fwd(C.byref(a), self._stream()), 'crit_tsum_fwd')

    def crit_tsum_bwd(self, words, theta, gamma, beta, fusion, adj, u, sent, fus, d_fus, dwords, part, eps=1e-5, p=0.0, site=0, seed=0,
                      row0=0, acc=None):
        """(adj, u, sent, fus of the forward are recomputed by the kernel: accepted for interface symmetry, not read)"""
        a = self._tsum_args(words, theta, gamma, beta, fusion, eps, p, site, seed, row0, acc)
        _chkc(d_fus); _chkc(dwords)
        a.d_fus, a.dwords, a.part = _p(d_fus), _p(dwords), _p(part)
        self._check(self.lib.dlsg_crit_tsum_bwd(C.byref(a), self._stream()), 'crit_tsum_bwd')

    def crit_tsum_bwd2(self, words, theta, gamma, beta, fusion, d_fus, U, Ufus, gwords, gpart, eps=1e-5, p=0.0, site=0, seed=0, row0=0):
        a = self._tsum_args(words, theta, gamma, beta, fusion, eps, p, site, seed, row0)
        for t in (d_fus, U, Ufus, gwords, gpart):
            _chkc(t)
        a.d_fus, a.U, a.Ufus, a.gwords, a.gpart = _p(d_fus), _p(U), _p(Ufus), _p(gwords), _p(gpart)
        self._check(self.lib.dlsg_crit_tsum_bwd2(C.byref(a), self._stream()), 'crit_tsum_bwd2')

    def _score_args(self, v, s, wc, wgt, fus, pair, score, ng, acc=None):
        a = abi.dlsg_crit_score_args()
        self._set2(a, v=v, s=s, wc=wc, wgt=wgt, pair=pair, score=score)
        _chkc(fus)
        a.fus = _p(fus)
        a.n, a.B, a.T, a.ng = s[0].shape[0], v[0].shape[0], v[0].shape[1], ng
        a.acc_lo, a.acc_hi = acc if acc is not None else (0, 0)
        return a

    def crit_score_fwd(self, v, s, wc, bc, wgt, fus, pair, score, both, out, ng):
        a = self._score_args(v, s, wc, wgt, fus, pair, score, ng)
        self._set2(a, bc=bc)
        _chkc(both); _chkc(out)
        a.both, a.out = _p(both), _p(out)
        self._check(self.lib.dlsg_crit_score_fwd(C.byref(a), self._stream()), 'crit_score_fwd')

    def crit_score_bwd(self, v, s, wc, wgt, fus, pair, score, both, d_out, d_fus, c_spre, c_vpre, d_wgt, part_wc, dbc, ng, acc=None):
        a = self._score_args(v, s, wc, wgt, fus, pair, score, ng, acc)
        self._set2(a, c_spre=c_spre, c_vpre=c_vpre, d_wgt=d_wgt, part_wc=part_wc)
        for t in (both, d_out, d_fus):
            _chkc(t)
        a.both, a.d_out, a.d_fus, a.dbc = _p(both), _p(d_out), _p(d_fus), _p(dbc)
        scratch = torch.empty(4 * ng + 16, dtype=torch.float32, device=fus.device)
        a.scratch = _p(scratch)
        self._check(self.lib.dlsg_crit_score_bwd(C.byref(a), self._stream()), 'crit_score_bwd')

    def crit_score_bwd2(self, v, s, wc, bc, wgt, fus, pair, score, d_out, Uspre, Uwgt, Ufus, g_fus, g_spre, g_vpre, g_wgt, gpart_wc, g_dbc):
        a = self._score_args(v, s, wc, wgt, fus, pair, score, 1)
        self._set2(a, Uspre=Uspre, Uwgt=Uwgt, c_spre=g_spre, c_vpre=g_vpre, d_wgt=g_wgt, part_wc=gpart_wc)
        for t in (d_out, Ufus, g_fus, g_dbc):
            _chkc(t)
        a.d_out, a.Ufus, a.d_fus, a.dbc = _p(d_out), _p(Ufus), _p(g_fus), _p(g_dbc)
        n = s[0].shape[0]
        scratch = torch.empty(16 + 2 * n + 2 * n * 8, dtype=torch.float32, device=fus.device)
        a.scratch = _p(scratch)
        self._check(self.lib.dlsg_crit_score_bwd2(C.byref(a), self._stream()), 'crit_score_bwd2')

    def crit_gp(self, g, gG, out, stats, vseed, gsc):
        B, L, _ = g.shape
        for t in (g, gG, out, stats, vseed, gsc):
            _chkc(t)
        q = torch.empty(B, dtype=torch.float32, device=g.device)
        self._check(self.lib.dlsg_crit_gp(_p(g), _p(gG), _p(out), _p(stats), _p(vseed), _p(gsc), _p(q), B, L, self._stream()), 'crit_gp')

    def crit_topk(self, alpha, smask, P, T, idx):
        B, L, na = alpha.shape
        assert alpha.stride(2) == 1 and alpha.dtype == torch.float32
        _chkc(smask); _chkc(idx)
        self._check(self.lib.dlsg_crit_topk(_p(alpha), i64(alpha.stride(0)), i64(alpha.stride(1)), na, _p(smask), _p(idx), B, L, P, T,
                                            self._stream()), 'crit_topk')

    def crit_unselect(self, src, idx, dst, per):
        """dst (R, n): row idx[r] = src[r], every other row zero; dst is groups of `per` rows, idx holds the selected rows of each
        group (the same number per group), group by group"""
        _chkc(src); _chkc(idx); _chkc(dst)
        self._check(self.lib.dlsg_crit_unselect(_p(src), _p(idx), _p(dst), src.shape[0], dst.shape[0], per, dst.shape[1], self._stream()),
                    'crit_unselect')

    def crit_reduce(self, descs):
        """descs: list of (slabs (S, ...) contiguous, out): out = sum over the S slabs, in slab order; one launch per 16"""
        for lo in range(0, len(descs), 16):
            chunk = descs[lo:lo + 16]
            arr = (abi.dlsg_crit_reduce_desc * len(chunk))()
            for d, (slabs, out) in zip(arr, chunk):
                _chkc(slabs); _chkc(out)
                assert out.numel() * slabs.shape[0] == slabs.numel() and out.numel() % 4 == 0
                d.src, d.stride, d.n, d.nslab, d.scale, d.out = _p(slabs), out.numel(), out.numel(), slabs.shape[0], 1.0, _p(out)
            self._check(self.lib.dlsg_crit_reduce(arr, len(chunk), self._stream()), 'crit_reduce')

    def crit_colsum(self, descs):
        """descs: list of (sources, out, out_b, scale): out = scale * sum over the rows of the one or two 2-d sources (unit column
        stride); out_b (or None) receives a copy.  One launch per 48 descriptors, fixed order of additions."""
        for lo in range(0, len(descs), 48):
            chunk = descs[lo:lo + 48]
            arr = (abi.dlsg_crit_colsum_desc * len(chunk))()
            for d, (srcs, out, out_b, scale) in zip(arr, chunk):
                a = srcs[0]
                assert a.dim() == 2 and (a.stride(1) == 1 or a.shape[1] == 1) and out.numel() == a.shape[1] and out.is_contiguous()
                d.part, d.ld, d.rows, d.n = _p(a), a.stride(0), a.shape[0], a.shape[1]
                if len(srcs) > 1:
                    b = srcs[1]
                    assert b.dim() == 2 and (b.stride(1) == 1 or b.shape[1] == 1) and b.shape[1] == a.shape[1]
                    d.part_b, d.ld_b, d.rows_b = _p(b), b.stride(0), b.shape[0]
                d.out, d.out_b, d.scale = _p(out), _p(out_b), scale
            self._check(self.lib.dlsg_crit_colsum(arr, len(chunk), self._stream()), 'crit_colsum')

    def gather_rows(self, src, idx, dst):
        """dst[r] = src[idx[r]] (2-d views; dst must not alias src)."""
        rows, n = dst.shape
        self._check(self.lib.dlsg_gather_rows(_p(src), i64(src.stride(0)), _p(idx), _p(dst), i64(dst.stride(0)), rows, n,
                                              self._stream()), 'gather_rows')

    def permute_tb(self, src, dst):
        """dst[b, t, :] = src[t, b, :]  (both contiguous 3-d)."""
        T, B, n = src.shape
        self._check(self.lib.dlsg_permute_tb(_p(src), _p(dst), T, B, n, self._stream()), 'permute_tb')

    # ------------------------------------------------------------------ loss / optimizer
    def ce_ragged(self, logits, targets, lens, dlogits, row_loss, loss, time_major):
        """logits (B,L,V) or, time_major, (L,B,V); targets (B,L) int64; lens (B,) int64."""
        if time_major:
            L, B, V = logits.shape
        else:
            B, L, V = logits.shape
        self._check(self.lib.dlsg_ce_ragged(_p(logits), _p(targets), _p(lens), _p(dlogits), _p(row_loss), _p(loss), B, L, V,
                                            int(time_major), self._stream()), 'ce_ragged')

    def ce_ragged_weighted(self, logits, targets, lens, weights, dlogits, row_loss, loss, time_major):
        """ce_ragged with caption b's rows weighted by weights[b] (float32 device tensor, (B,))"""
        if time_major:
            L, B, V = logits.shape
        else:
            B, L, V = logits.shape
        assert weights.dtype == torch.float32 and weights.numel() == B and weights.is_contiguous()
        self._check(self.lib.dlsg_ce_ragged_weighted(_p(logits), _p(targets), _p(lens), _p(weights), _p(dlogits), _p(row_loss), _p(loss),
                                                     B, L, V, int(time_major), self._stream()), 'ce_ragged_weighted')

    def ce_ragged_soft(self, logits, targets, lens, dlogits, row_loss, loss, time_major, smoothing=0.0, weights=None, teachers=(),
                       teacher_weights=None, mode=0, alpha=0.0):
        """ce_ragged against the soft target row (1 - alpha) * ((1 - smoothing) * onehot + smoothing / V) + alpha * q, q the word
        distribution of `teachers` -- a sequence of float32 logits arrays of the shape and row order of `logits` (rows may be
        strided), combined with `teacher_weights` (positive, default uniform, normalised here in float64) by `mode` 0 (weighted mean
        probability) or 1 (weighted geometric mean, renormalised); see include/dlsg.h.  weights: optional (B,) float32 per caption.
        row_loss: scratch of 3 * B * L floats; loss: 3 floats {mixed loss, NLL of the targets, CrossEntropy against q}."""
        if time_major:
            L, B, V = logits.shape
        else:
            B, L, V = logits.shape
        M = len(teachers)
        assert logits.dtype == dlogits.dtype == torch.float32 and logits.is_contiguous() and dlogits.is_contiguous()
        assert dlogits.shape == logits.shape, (dlogits.shape, logits.shape)
        assert targets.dtype == torch.int64 and targets.is_contiguous() and targets.shape == (B, L), (targets.dtype, targets.shape)
        assert lens.dtype == torch.int64 and lens.is_contiguous() and lens.numel() == B
        assert row_loss.dtype == torch.float32 and row_loss.is_contiguous() and row_loss.numel() >= 3 * B * L
        assert loss.dtype == torch.float32 and loss.is_contiguous() and loss.numel() == 3
        assert weights is None or (weights.dtype == torch.float32 and weights.numel() == B and weights.is_contiguous())
        ptrs = lds = ws = logws = None
        if M:
            w = normalised_weights([1.0] * M if teacher_weights is None else teacher_weights)
            assert len(w) == M, (len(w), M)
            rows = []
            for x in teachers:
                assert x.dtype == torch.float32 and x.shape == logits.shape and x.device == logits.device, (x.dtype, x.shape)
                x2 = x.view(B * L, V) if x.is_contiguous() else x.reshape(B * L, V)
                assert x2.data_ptr() == x.data_ptr() and (x2.stride(1) == 1 or V == 1), 'teacher rows must be equally strided, unit column stride'
                rows.append(x2)
            ptrs = (C.c_void_p * M)(*[x.data_ptr() for x in rows])
            lds = (C.c_int64 * M)(*[x.stride(0) for x in rows])
            ws = (C.c_float * M)(*w)
            logws = (C.c_float * M)(*[math.log(x) for x in w])
        self._check(self.lib.dlsg_ce_ragged_soft(_p(logits), _p(targets), _p(lens), _p(weights), _p(dlogits), _p(row_loss), _p(loss),
                                                 B, L, V, int(time_major), f32(smoothing), f32(alpha), ptrs, lds, ws, logws, M, int(mode),
                                                 self._stream()), 'ce_ragged_soft')

    @staticmethod
    def _risk_shape(logits, targets, lens, lse, tok_lp, n, time_major):
        if time_major:
            L, rows, V = logits.shape
        else:
            rows, L, V = logits.shape
        assert logits.dtype == torch.float32 and logits.is_contiguous(), (logits.dtype, logits.stride())
        assert targets.dtype == torch.int64 and targets.is_contiguous() and targets.shape == (rows, L), (targets.dtype, targets.shape)
        assert lens.dtype == torch.int64 and lens.is_contiguous() and lens.numel() == rows
        for x in (lse, tok_lp):
            assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == rows * L, (x.dtype, x.shape)
        assert int(n) == n, n
        return rows, L, V

    def risk_rows(self, logits, targets, lens, lse, tok_lp, n, time_major):
        """the first launch of the minimum-risk loss (include/addons/dlsg_risk.h): lse and tok_lp (rows * L float32, the logits' row
        order) of logits (rows, L, V) or, time_major, (L, rows, V); targets (rows, L) int64; lens (rows,) int64; n candidates per clip"""
        rows, L, V = self._risk_shape(logits, targets, lens, lse, tok_lp, n, time_major)
        self._check(self.lib.dlsg_risk_rows(_p(logits), _p(targets), _p(lens), _p(lse), _p(tok_lp), rows, int(n), L, V, int(time_major),
                                            self._stream()), 'risk_rows')

    def risk_grad(self, logits, targets, lens, lse, tok_lp, rewards, valid, dlogits, Q, s, R, loss, stats, n, time_major, alpha,
                  length_penalty=0.0):
        """the second launch, on what `risk_rows` wrote for the same logits: dlogits (as logits), Q and s (rows,) float64, R (rows / n,)
        float64, loss (1,) float32, stats (4,) float64 {loss, mean reward and mean length of the counted candidates, mean R_b}.
        rewards (rows,) float64; valid (rows,) bool or uint8, or None."""
        rows, L, V = self._risk_shape(logits, targets, lens, lse, tok_lp, n, time_major)
        assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and dlogits.shape == logits.shape, (dlogits.dtype, dlogits.shape)
        assert rewards.dtype == torch.float64 and rewards.is_contiguous() and rewards.numel() == rows, (rewards.dtype, rewards.shape)
        assert valid is None or (valid.dtype in (torch.bool, torch.uint8) and valid.is_contiguous() and valid.numel() == rows)
        for x in (Q, s):
            assert x.dtype == torch.float64 and x.is_contiguous() and x.numel() == rows, (x.dtype, x.shape)
        assert R.dtype == torch.float64 and R.is_contiguous() and int(n) >= 1 and R.numel() >= rows // int(n), (R.dtype, R.shape, rows, n)
        assert loss.dtype == torch.float32 and loss.is_contiguous() and loss.numel() == 1
        assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == 4
        self._check(self.lib.dlsg_risk_grad(_p(logits), _p(targets), _p(lens), _p(lse), _p(tok_lp), _p(rewards), _p(valid), _p(dlogits),
                                            _p(Q), _p(s), _p(R), _p(loss), _p(stats), rows, int(n), L, V, int(time_major), float(alpha),
                                            float(length_penalty), self._stream()), 'risk_grad')

    def cider_d(self, ids, clip_idx, end_id, tables, out):
        """out[r] (float64) = CIDEr-D of the words of ids[r] (int64 (R, L), L <= 64, unit column stride; the words before the first
        end_id) against the references of clip clip_idx[r] (int32) in `tables` (a scoring.DeviceCiderD)"""
        R, L = ids.shape
        assert ids.dtype == torch.int64 and (ids.stride(1) == 1 or L <= 1), (ids.dtype, ids.stride())
        assert clip_idx.dtype == torch.int32 and clip_idx.is_contiguous() and clip_idx.numel() == R
        assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == R
        self._check(self.lib.dlsg_cider_d(_p(ids), i64(ids.stride(0)), R, L, _p(clip_idx), i64(end_id), C.byref(cider_tables(tables)),
                                          _p(out), self._stream()), 'cider_d')

    def cider_consensus(self, ids, end_id, tables, scores, temperature, util, expected, order):
        """consensus ranking of the n candidates ids[b] (int64 (B, n, L), n <= 32, L <= 64, unit word stride, candidate rows
        equally strided over the whole batch) by CIDEr-D against each other on the corpus idf of `tables` (a scoring.DeviceCiderD):
        expected (float64 (B, n)) the expected utility of a candidate over the others, weighted exp((scores - max) / temperature)
        (scores float32 (B, n), None: uniform), order (int64 (B, n)) its descending ranking, util (float64 (B, n, n) or None) the
        pairwise utilities.  See dlsg_cider_consensus in include/dlsg.h."""
        assert ids.dim() == 3 and ids.dtype == torch.int64, (ids.dtype, ids.shape)
        B, n, L = ids.shape
        ld = max(ids.stride(1), L) if B * n <= 1 else ids.stride(1) if n > 1 else ids.stride(0)      # candidate b n + i at (b n + i) ld
        assert (ids.stride(2) == 1 or L <= 1) and (ids.stride(0) == n * ld or B <= 1 or n <= 1) and ld >= L, ids.stride()
        assert scores is None or (scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (B, n))
        assert util is None or (util.dtype == torch.float64 and util.is_contiguous() and util.shape == (B, n, n))
        assert expected.dtype == torch.float64 and expected.is_contiguous() and expected.shape == (B, n)
        assert order.dtype == torch.int64 and order.is_contiguous() and order.shape == (B, n)
        self._check(self.lib.dlsg_cider_consensus(_p(ids), i64(ld), B, n, L, i64(end_id),
                                                  C.byref(cider_tables(tables)), _p(scores), float(temperature), _p(util),
                                                  _p(expected), _p(order), self._stream()), 'cider_consensus')

    def caption_metrics(self, ids, clip_idx, end_id, tables, scores=None, stats=None, reward=None, weights=None, base=None):
        """BLEU-1..4 and ROUGE_L of the words of ids[r] (as in `cider_d`) against the references of clip clip_idx[r] in `tables` (a
        scoring.DeviceCaptionMetrics).  Outputs, each optional: scores (float64 (R, 5)), stats (int32 (R, 10): correct[4], guess[4],
        length, closest reference length), reward (float64 (R,)) = weights[0] base + weights[1..4] BLEU-1..4 + weights[5] ROUGE_L
        with weights a sequence of 6 host floats and base float64 (R,) (needed only when weights[0] != 0)"""
        R, L = ids.shape
        assert ids.dtype == torch.int64 and (ids.stride(1) == 1 or L <= 1), (ids.dtype, ids.stride())
        assert clip_idx.dtype == torch.int32 and clip_idx.is_contiguous() and clip_idx.numel() == R
        assert scores is None or (scores.dtype == torch.float64 and scores.is_contiguous() and scores.shape == (R, 5))
        assert stats is None or (stats.dtype == torch.int32 and stats.is_contiguous() and stats.shape == (R, 10))
        assert reward is None or (reward.dtype == torch.float64 and reward.is_contiguous() and reward.numel() == R)
        assert base is None or (base.dtype == torch.float64 and base.is_contiguous() and base.numel() == R)
        assert tables.ref_words.dtype == torch.int16 and tables.clip_off.dtype == tables.ref_off.dtype == torch.int64
        w = None
        if reward is not None:
            assert weights is not None and len(weights) == 6 and (base is not None or float(weights[0]) == 0.0)
            w = (C.c_double * 6)(*[float(x) for x in weights])
        self._check(self.lib.dlsg_caption_metrics(_p(ids), i64(ids.stride(0)), R, L, _p(clip_idx), i64(end_id), _p(tables.clip_off),
                                                  _p(tables.ref_off), _p(tables.ref_words), tables.n_clips, tables.V, w, _p(base),
                                                  _p(scores), _p(stats), _p(reward), self._stream()), 'caption_metrics')

    def caption_corpus(self, stats, scores, base, out):
        """out (float64 (6,)) = corpus BLEU-1..4 from the column sums of stats (int32 (R, 10)), the mean of scores[:, 4] (ROUGE_L;
        scores float64 (R, 5)) and the mean of base (float64 (R,), None: NaN); R >= 1"""
        R = stats.shape[0]
        assert stats.dtype == torch.int32 and stats.is_contiguous() and stats.shape == (R, 10)
        assert scores.dtype == torch.float64 and scores.is_contiguous() and scores.shape == (R, 5)
        assert base is None or (base.dtype == torch.float64 and base.is_contiguous() and base.numel() == R)
        assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 6
        self._check(self.lib.dlsg_caption_corpus(_p(stats), _p(scores), _p(base), R, _p(out), self._stream()), 'caption_corpus')

    def scst_advantage(self, rewards, lens, greedy, n, adv, stats):
        """adv = (float32) rewards - baseline over B clips x n samples: greedy[b] (float64 (B,)) or, greedy None, the leave-one-out
        mean of the clip's other samples; stats (float64 (3,)) = mean reward, mean baseline, mean of lens (int64)"""
        N = rewards.numel()
        assert n >= 1 and N % n == 0 and rewards.dtype == torch.float64 and rewards.is_contiguous()
        assert lens.dtype == torch.int64 and lens.is_contiguous() and lens.numel() == N
        assert greedy is None or (greedy.dtype == torch.float64 and greedy.is_contiguous() and greedy.numel() == N // n)
        assert adv.dtype == torch.float32 and adv.is_contiguous() and adv.numel() == N
        assert stats.dtype == torch.float64 and stats.numel() == 3
        self._check(self.lib.dlsg_scst_advantage(_p(rewards), _p(lens), _p(greedy), N // n, int(n), _p(adv), _p(stats), self._stream()),
                    'scst_advantage')

    def log_softmax(self, logits, out):
        rows, V = logits.shape
        self._check(self.lib.dlsg_log_softmax(_p(logits), _p(out), rows, V, self._stream()), 'log_softmax')

    def adam(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, hyper=None):
        """hyper: optional device tensor {lr/(1-b1^step), sqrt(1-b2^step)} read at run time (graph replay).  The launch is guarded
        by the persistent kernels' time-out word of this device: a step whose recurrent hand-off timed out (gradients invalid)
        updates nothing; `check_persistent()` then reports it."""
        self._check(self.lib.dlsg_adam(_p(p), _p(g), _p(m), _p(v), i64(p.numel()), f32(lr), f32(b1), f32(b2), f32(eps),
                                       int(step), f32(grad_scale), _p(hyper), _p(self._persist_word(p.device)), self._stream()), 'adam')

    # ------------------------------------------------------------------ gradient clipping (include/dlsg.h)
    def grad_sumsq(self, g, slots):
        """slots (float64, GRAD_SUMSQ_SLOTS) <- the partial sums of g^2 over the 1-d float32 view g, one per workgroup; every slot
        is written (zeros where a workgroup had nothing), none needs clearing first"""
        assert g.dtype == torch.float32 and g.dim() == 1 and (g.numel() <= 1 or g.stride(0) == 1), (g.dtype, g.shape)
        assert slots.dtype == torch.float64 and slots.is_contiguous() and slots.numel() == GRAD_SUMSQ_SLOTS, (slots.dtype, slots.shape)
        self._check(self.lib.dlsg_grad_sumsq(_p(g), i64(g.numel()), _p(slots), self._stream()), 'grad_sumsq')

    def clip_coef(self, slots, grad_scale, max_norm, record, skipped=None):
        """record (float32, CLIP_RECORD_FLOATS) <- {norm = grad_scale * sqrt(sum of slots), coef = min(1, max_norm / (norm + 1e-6)),
        nonfinite}; a non-finite norm gives coef 0 and adds one to skipped (int64, 1 element).  max_norm = inf clips nothing."""
        assert slots.dtype == torch.float64 and slots.is_contiguous() and 1 <= slots.numel() < 2 ** 31
        assert record.dtype == torch.float32 and record.is_contiguous() and record.numel() == CLIP_RECORD_FLOATS
        assert skipped is None or (skipped.dtype == torch.int64 and skipped.numel() == 1)
        self._check(self.lib.dlsg_clip_coef(_p(slots), int(slots.numel()), f32(grad_scale), f32(max_norm), _p(record), _p(skipped),
                                            self._stream()), 'clip_coef')

    def adam_clipped(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, hyper=None, record=None, clip_value=0.0):
        """`adam` on (g * grad_scale) * record[CLIP_COEF], clamped to +-clip_value when that is > 0; a record whose nonfinite word is
        set leaves p, m and v as they are (as the time-out word does)"""
        assert record is None or (record.dtype == torch.float32 and record.is_contiguous() and record.numel() == CLIP_RECORD_FLOATS)
        self._check(self.lib.dlsg_adam_clipped(_p(p), _p(g), _p(m), _p(v), i64(p.numel()), f32(lr), f32(b1), f32(b2), f32(eps),
                                               int(step), f32(grad_scale), _p(hyper), _p(self._persist_word(p.device)), _p(record),
                                               f32(clip_value), self._stream()), 'adam_clipped')

    # ------------------------------------------------------------------ weight decay and averaged weights (include/dlsg.h)
    def adamw_ema(self, p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0, weight_decay=0.0, decoupled=True, ema=None, ema_decay=0.0,
                  hyper=None, record=None, clip_value=0.0, decay_ranges=None):
        """`adam_clipped` with weight decay (decoupled: p *= 1 - lr * weight_decay in front of the update, AdamW; else
        g += weight_decay * p behind the clip, Adam's L2) and, with ema (float32, laid out as p), ema += (1 - ema_decay) * (p_new - ema).
        hyper: optional device tensor of FOUR floats {lr/(1-b1^step), sqrt(1-b2^step), 1 - lr*wd (decoupled) or wd, 1 - ema_decay}.
        decay_ranges: optional device int64 (k, 2), sorted disjoint [lo, hi) element intervals of p that are decayed (None: all of
        it), k <= ADAM_MAX_RANGES.  A skipped step (time-out word, non-finite record) leaves p, m, v and ema as they are."""
        assert record is None or (record.dtype == torch.float32 and record.is_contiguous() and record.numel() == CLIP_RECORD_FLOATS)
        assert hyper is None or (hyper.dtype == torch.float32 and hyper.numel() == 4 and hyper.is_contiguous()), 'hyper holds four floats'
        assert ema is None or (ema.dtype == torch.float32 and ema.shape == p.shape and ema.device == p.device)
        k = 0
        if decay_ranges is not None:
            assert decay_ranges.dtype == torch.int64 and decay_ranges.dim() == 2 and decay_ranges.shape[1] == 2 \
                and decay_ranges.is_contiguous() and decay_ranges.device == p.device, (decay_ranges.dtype, decay_ranges.shape)
            k = decay_ranges.shape[0]
        self._check(self.lib.dlsg_adamw_ema(_p(p), _p(g), _p(m), _p(v), _p(ema), i64(p.numel()), f32(lr), f32(b1), f32(b2), f32(eps),
                                            int(step), f32(grad_scale), f32(weight_decay), int(bool(decoupled)), f32(ema_decay),
                                            _p(hyper), _p(self._persist_word(p.device)), _p(record), f32(clip_value),
                                            _p(decay_ranges) if k else None, int(k), self._stream()), 'adamw_ema')

    def swap(self, a, b):
        """a <-> b in place: two 1-d float32 views of equal length"""
        assert a.dtype == b.dtype == torch.float32 and a.dim() == b.dim() == 1 and a.numel() == b.numel() and a.device == b.device
        assert (a.numel() <= 1 or a.stride(0) == 1) and (b.numel() <= 1 or b.stride(0) == 1)
        self._check(self.lib.dlsg_swap_f32(_p(a), _p(b), i64(a.numel()), self._stream()), 'swap')
