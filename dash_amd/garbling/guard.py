"""Exact run-time range guard of the garbler's inputs (the mixed-radix rescale's wrap band, CRT overflow).

The garbled circuit computes every value modulo M = prod(CRT base) and its non-linear gadgets read them as
signed values in [-M/2, M/2). Two constructions are exact only on a narrower range:

* the mixed-radix rescale (gadgets.h RescaleMrsPlan) adds U = M/2 rounded up to S - 1 mod S (S = 2^l) before
  its single conversion, so its inputs must stay below ``Rescale.mrs_limit(M)``: the top < 2^l values below
  M/2 wrap and decode to a wrong but *valid* label (docs/SECURITY.md "mixed-radix wrap band");
* every gadget input outside [-M/2, M/2) has already wrapped modulo M (CRT overflow) — the reference's own
  failure mode, which it only guards statically through range calibration (circuit.h:159-265,
  rescale_gadget.h:115-242 is exact on the whole signed range but not beyond it).

The garbler knows its plaintext input and the public weights, so it can decide exactly, per input, whether
the garbled result will equal the plaintext one: it evaluates the quantized model and checks the input of
every non-linear gadget (ReLU, Sign, MaxPool, Rescale) and the outputs. An input that fails is refused with
``RangeGuardError`` before its result is released (never a silently wrong label).

Max pooling is a pairwise tree of max(a, b) = a + relu(b - a): besides its inputs, every difference b - a it
feeds a ReLU gadget must be a signed value. The guard bounds them all by the window's span: max - min <=
min(M/2, M - M/2 - 1) (a sufficient condition, exact for the tree's pairs).

Three implementations with one semantics (tests/test_range_guard.py pins them against each other):

* on a GPU, ``DevRangeGuard`` (csrc/hip/guard.hip): one HIP launch per layer over chunks of the batch,
  int64 activations and 32 x 32 -> 64-bit products, on its own high-priority stream beside the garbled
  evaluation; inputs whose activations exceed a kernel's exact operand range (int32, or the 24-bit conv form's
  bound) are marked uncertain and decided by the numpy model alone, whatever the device flagged for them. It
  has no Concat, no Clip, no ArgMax, no Mul, no MatMul, no ConvTranspose2d, no Upsample, no LeakyRelu, no
  PiecewiseLinear, no Gather, no Bilinear and no padded / ceil-mode pooling:
  circuits with any of them take the torch path on the GPU;
* the batched torch evaluation (float64 GEMMs, exact below 2^53), used on the CPU and as the bench's batched
  verification oracle (``outputs``);
* the per-input numpy model (``violations_np``), the exact reference of both and the path of layers without a
  batched form (test-only Mult / Max).

A ``Mul`` sets no limit of its own: its product is checked where a gadget or the output next reads it. The torch
path multiplies in int64, exact like the numpy model; operands whose product could reach 2^62, where the numpy
model raises ``OverflowError`` instead of wrapping, are flagged. A ``MatMul`` is treated the same way: no limit
of its own, an int64 broadcast multiply and sum over the contracted axis in the torch path (no int64 matmul exists
on the GPU), operands whose T products could sum to 2^62 flagged; guard.hip has none, so such circuits take the
torch path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from ..ir import layers as L


class RangeGuardError(ValueError):
    """A garbler input whose garbled evaluation would leave a gadget's exact range (wrap band / overflow)."""


def _half(M: int) -> int:
    return M // 2


class RangeGuard:
    """Per-circuit exact range check. ``mrs=True``: DASH Rescale(l) inputs must stay below the mixed-radix
    wrap band; every gadget input and output must be a signed CRT value in [-M/2, M/2)."""

    CHUNK = 16  # inputs per GPU pass (im2col working set ~60 MB on the MiniONN CNN)

    def __init__(self, circuit, crt_modulus: int, mrs: bool = True, device: Optional[int] = None,
                 joint_clips: Optional[dict] = None):
        """joint_clips: {layer index: t_hi} of the Clips garbled with the joint construction (gadgets.h ClipPlan):
        their upper sign reads the input x of the rescale before them, so that rescale needs x >= -M/2 + t_hi,
        and the Clip's own input only has to be a signed CRT value."""
        self.circuit, self.M, self.mrs = circuit, int(crt_modulus), bool(mrs)
        self.joint_clips = {int(i): int(t) for i, t in (joint_clips or {}).items()}
        self.device = device
        self.batched = all(isinstance(l, (L.Conv2d, L.Dense, L.Rescale, L.Relu, L.Sign, L.Flatten, L.MaxPool2d,
                                          L.SumPool2d, L.Add, L.Concat, L.Clip, L.ArgMax, L.Mul, L.Projection,
                                          L.BaseExtension, L.ConvTranspose2d, L.Upsample, L.LeakyRelu,
                                          L.PiecewiseLinear, L.MatMul, L.Gather, L.Bilinear))
                           for l in circuit.layers)
        # DevRangeGuard (guard.hip) has no Concat, no Clip, no ArgMax, no Mul, no ConvTranspose2d, no Upsample, no
        # LeakyRelu, no PiecewiseLinear, no MatMul, no Gather, no Bilinear, no dilated conv and no padded / ceil-mode
        # pooling: such circuits take the batched torch path
        self.native_forms = not any(isinstance(l, (L.Concat, L.Clip, L.ArgMax, L.Mul, L.ConvTranspose2d, L.Upsample,
                                                   L.LeakyRelu, L.PiecewiseLinear, L.MatMul, L.Gather, L.Bilinear)) or
                                    (isinstance(l, L.Conv2d) and (l.dh > 1 or l.dw > 1)) or
                                    (isinstance(l, (L.MaxPool2d, L.SumPool2d)) and l.padded) for l in circuit.layers)
        self._w = None
        self._stream = None
        self._dev = None  # DevRangeGuard (GPU), built on first use

    # ------------------------------------------------------------------ limits
    def _limits(self, layer) -> Optional[tuple]:
        """(lo, hi_exclusive) the layer's input must satisfy, or None (linear / free layers)."""
        h = _half(self.M)
        lo, hi = -h, self.M - h
        idx = next((i for i, l in enumerate(self.circuit.layers) if l is layer), -1) if self.joint_clips else -1
        if isinstance(layer, L.Rescale):
            if self.mrs and layer.use_sign_base_extension and layer.l >= 1:
                hi = min(hi, layer.mrs_limit(self.M))
            if idx + 1 in self.joint_clips:  # the joint Clip's upper sign input x - t_hi is a signed CRT value
                lo = lo + self.joint_clips[idx + 1]
            return lo, hi
        # a LeakyRelu's sign reads its input; its output 2^s x is checked where a gadget or the output next reads it
        if isinstance(layer, (L.Relu, L.Sign, L.MaxPool2d, L.Max, L.ArgMax, L.LeakyRelu)):
            return lo, hi
        if isinstance(layer, L.Clip):
            if idx in self.joint_clips:  # its signs were taken at the rescale before it
                return lo, hi
            # both sign inputs x - q_lo and x - q_hi are signed CRT values
            return lo + layer.q_hi, hi + layer.q_lo
        if isinstance(layer, L.PiecewiseLinear):  # every sign input x - T_i is a signed CRT value
            return lo + int(layer.T[-1]), hi + int(layer.T[0])
        return None

    def span_max(self) -> int:
        """Largest max - min of a max-pooling window (or of an ArgMax's candidates) whose pairwise differences
        are all signed CRT values."""
        h = _half(self.M)
        return min(h, self.M - h - 1)

    # ------------------------------------------------------------------ exact per-input reference (numpy)
    def violations_np(self, x) -> list:
        """[(layer index or 'out', min, max, lo, hi)] of one input, by the numpy plaintext evaluation."""
        c, M = self.circuit, self.M
        x = np.asarray(x, dtype=np.int64).reshape(-1)
        ctx, cur, bad = [x], x, []
        for i, l in enumerate(c.layers):
            src = getattr(l, "in_src", None)
            inp = ctx[src + 1] if src is not None else cur
            lim = self._limits(l)
            if lim is not None and inp.size:
                mn, mx = int(inp.min()), int(inp.max())
                if mn < lim[0] or mx >= lim[1]:
                    bad.append((i, mn, mx, lim[0], lim[1]))
            if isinstance(l, L.MaxPool2d) and inp.size:
                w = np.stack(l._windows(inp))
                span = int((w.max(axis=0) - w.min(axis=0)).max())
                if span > self.span_max():
                    bad.append((i, "span", span, 0, self.span_max()))
            if isinstance(l, L.ArgMax) and inp.size:
                v = inp.reshape(l.K, l.P)
                span = int((v.max(axis=0) - v.min(axis=0)).max())
                if span > self.span_max():
                    bad.append((i, "span", span, 0, self.span_max()))
            try:
                cur = l.plain_q_eval(inp, False, ctx, M)
            except OverflowError:  # a Mul whose product leaves int64: far beyond any signed CRT value
                bad.append((i, "overflow", 0, -_half(M), M - _half(M)))
                return bad
            ctx.append(cur)
        h = _half(M)
        if cur.size and (int(cur.min()) < -h or int(cur.max()) >= M - h):
            bad.append(("out", int(cur.min()), int(cur.max()), -h, M - h))
        return bad

    # ------------------------------------------------------------------ batched torch path
    def _tdev(self):
        import torch

        if self.device is not None and torch.cuda.is_available():
            return torch.device("cuda", int(self.device))
        return torch.device("cpu")

    def _weights(self, dev):
        import torch

        if self._w is None or self._w[0] != dev:
            ws = []
            for l in self.circuit.layers:
                if isinstance(l, L.Conv2d):
                    ws.append((torch.tensor(np.array(l.q_weights.reshape(l.F, -1)), dtype=torch.float64, device=dev),
                               torch.tensor(np.array(l.q_biases), dtype=torch.float64, device=dev)))
                elif isinstance(l, L.ConvTranspose2d):  # [F kh kw][C]: the columns that fold sums into the output
                    ws.append((torch.tensor(np.array(l.q_weights.reshape(l.C, -1).T), dtype=torch.float64, device=dev),
                               torch.tensor(np.array(l.q_biases), dtype=torch.float64, device=dev)))
                elif isinstance(l, L.Dense):
                    perm = None
                    if l.channel_tf:
                        K, ch = l.in_size, l.channel_tf
                        i = np.arange(K)
                        perm = torch.as_tensor(i // ch + (i % ch) * (K // ch), device=dev)
                    ws.append((torch.tensor(np.array(l.q_weights), dtype=torch.float64, device=dev),
                               torch.tensor(np.array(l.q_biases), dtype=torch.float64, device=dev), perm))
                elif isinstance(l, L.Gather):
                    ws.append(torch.as_tensor(np.array(l.idx), device=dev))
                elif isinstance(l, L.Bilinear):  # taps and the four weight vectors, int64
                    ws.append(tuple(torch.as_tensor(np.array(a), device=dev) for a in (
                        l.y0, l.y1, (1 << l.by) - l.ny, l.ny, l.x0, l.x1, (1 << l.bx) - l.nx, l.nx)))
                else:
                    ws.append(None)
            self._w = (dev, ws)
        return self._w[1]

    def _bad_batch(self, X, want_out: bool = False):
        """X: (B, N) int64 tensor -> (B,) bool tensor, True where a gadget input leaves its exact range (and the
        outputs, with want_out)."""
        import torch
        import torch.nn.functional as F

        M, h = self.M, _half(self.M)
        ws = self._weights(X.device)
        B = X.shape[0]
        bad = torch.zeros(B, dtype=torch.bool, device=X.device)
        ctx, cur = [X], X
        for i, l in enumerate(self.circuit.layers):
            src = getattr(l, "in_src", None)
            inp = ctx[src + 1] if src is not None else cur
            lim = self._limits(l)
            if lim is not None:
                bad |= (inp < lim[0]).any(dim=1) | (inp >= lim[1]).any(dim=1)
            if isinstance(l, L.Conv2d):
                W, b = ws[i]
                cols = F.unfold(inp.to(torch.float64).view(B, l.C, l.H, l.W), (l.kh, l.kw), padding=(l.ph, l.pw),
                                stride=(l.sh, l.sw), dilation=(l.dh, l.dw))
                if l.groups == 1:
                    y = torch.matmul(W, cols) + b[:, None]
                else:  # grouped unfold: the group's filters against the group's own rows of cols
                    g = l.groups
                    y = torch.matmul(W.view(1, g, l.F // g, -1), cols.view(B, g, W.shape[1], -1))
                    y = y.reshape(B, l.F, -1) + b[:, None]
                out = y.reshape(B, -1).to(torch.int64)
            elif isinstance(l, L.ConvTranspose2d):
                W, b = ws[i]
                cols = torch.matmul(W, inp.to(torch.float64).view(B, l.C, l.H * l.W))
                y = F.fold(cols, (l.OH, l.OW), (l.kh, l.kw), padding=(l.ph, l.pw), stride=(l.sh, l.sw))
                out = (y + b[None, :, None, None]).reshape(B, -1).to(torch.int64)
            elif isinstance(l, L.Upsample):
                v = inp.view(B, l.C, l.H, l.W)
                out = v.repeat_interleave(l.fh, dim=2).repeat_interleave(l.fw, dim=3).reshape(B, -1)
            elif isinstance(l, L.Gather):  # sets no limit: the moved values are checked where a gadget next reads them
                out = inp.index_select(1, ws[i])
            elif isinstance(l, L.Bilinear):  # exact in int64 (index_select and integer multiplies); no limit of its own
                y0, y1, wy0, wy1, x0, x1, wx0, wx1 = ws[i]
                v = inp.view(B, l.C, l.H, l.W)
                r = v.index_select(2, y0) * wy0[None, None, :, None] + v.index_select(2, y1) * wy1[None, None, :, None]
                out = (r.index_select(3, x0) * wx0 + r.index_select(3, x1) * wx1).reshape(B, -1)
            elif isinstance(l, L.Dense):
                W, b, perm = ws[i]
                xin = inp if perm is None else inp[:, perm]
                out = (xin.to(torch.float64) @ W.t() + b).to(torch.int64)
            elif isinstance(l, L.Rescale):
                if l.use_sign_base_extension:
                    out = inp
                    for _ in range(l.l):
                        out = torch.div(out + h % 2, 2, rounding_mode="floor")
                else:
                    S = int(np.prod(l.s))
                    out = torch.div(inp + h % S, S, rounding_mode="floor")
            elif isinstance(l, L.Relu):
                out = torch.clamp_min(inp, 0)
            elif isinstance(l, L.LeakyRelu):
                n = torch.as_tensor(np.repeat(l.n, l.bc) if l.n.size > 1 else l.n, device=X.device)
                out = torch.where(inp >= 0, inp * (1 << l.slope_bits), inp * n[None, :])
            elif isinstance(l, L.PiecewiseLinear):
                out = int(l.V) + int(l.A[0]) * (inp - int(l.T[0]))
                for T, D in zip(l.T, l.D):
                    out = out + int(D) * torch.clamp_min(inp - int(T), 0)
            elif isinstance(l, L.Sign):
                out = torch.where(inp >= 0, 1, -1).to(torch.int64)
            elif isinstance(l, L.Clip):
                out = torch.clamp(inp, l.q_lo, l.q_hi)
            elif isinstance(l, L.ArgMax):
                v = inp.view(B, l.K, l.P)
                bad |= ((v.amax(dim=1) - v.amin(dim=1)) > self.span_max()).any(dim=1)
                out = torch.argmax(v, dim=1)  # the first of equal maxima, as np.argmax
            elif isinstance(l, L.MaxPool2d):
                v = inp.view(B, l.C, l.H, l.W)
                out = mn = None
                for dy in range(l.kh):
                    for dx in range(l.kw):
                        if l.padded:  # a tap outside the image reads the clamped coordinate (layers.MaxPool2d)
                            ys, xs = l._coords(dy, dx)
                            ys = torch.as_tensor(np.clip(ys, 0, l.H - 1), device=X.device)
                            xs = torch.as_tensor(np.clip(xs, 0, l.W - 1), device=X.device)
                            w = v[:, :, ys[:, None], xs[None, :]]
                        else:
                            w = v[:, :, dy:dy + l.sh * (l.OH - 1) + 1:l.sh, dx:dx + l.sw * (l.OW - 1) + 1:l.sw]
                        out = w if out is None else torch.maximum(out, w)
                        mn = w if mn is None else torch.minimum(mn, w)
                bad |= ((out - mn).reshape(B, -1) > self.span_max()).any(dim=1)
                out = out.reshape(B, -1)
            elif isinstance(l, L.SumPool2d):
                v = inp.view(B, l.C, l.H, l.W)
                if l.padded:  # zero padding up to the last window's end: skipped taps add nothing
                    eh = max(0, (l.OH - 1) * l.sh + l.kh - l.ph - l.H)
                    ew = max(0, (l.OW - 1) * l.sw + l.kw - l.pw - l.W)
                    v = F.pad(v, (l.pw, ew, l.ph, eh))
                out = 0
                for dy in range(l.kh):
                    for dx in range(l.kw):
                        out = out + v[:, :, dy:dy + l.sh * (l.OH - 1) + 1:l.sh, dx:dx + l.sw * (l.OW - 1) + 1:l.sw]
                out = out.reshape(B, -1)
            elif isinstance(l, L.Add):
                out = inp + ctx[l.src + 1]
            elif isinstance(l, L.Mul):
                y = inp if l.src is None else ctx[l.src + 1].reshape(B, -1)
                if l.bc:
                    y = y.repeat_interleave(l.bc, dim=1)
                # int64 products are exact below 2^63; where the numpy model raises OverflowError (2^62) the
                # input is flagged and the operands are zeroed so nothing wraps
                # max|x| max|y| >= 2^62 in exact integers: ax > floor((2^62 - 1) / ay)
                ax, ay = inp.abs().amax(dim=1), y.abs().amax(dim=1)
                big = (ay > 0) & (ax > torch.div((1 << 62) - 1, ay.clamp_min(1), rounding_mode="floor"))
                bad |= big
                out = torch.where(big[:, None], 0, inp) * y
            elif isinstance(l, L.MatMul):
                # per head: [B][G][M][T] and [B][G][T][N] (G = 1 for the single contraction)
                a = inp.reshape((B, l.heads) + L._head_matrix(l.in_dims, l.heads))
                y = ctx[l.src + 1].reshape((B, l.heads) + L._head_matrix(l.src_dims, l.heads))
                a = a.transpose(2, 3) if l.trans_a else a
                y = y.transpose(2, 3) if l.trans_b else y
                # T max|x| max|y| >= 2^62 in exact integers: ax > floor(floor((2^62 - 1) / T) / ay). Such inputs are
                # flagged (the numpy model raises OverflowError) and their x zeroed so nothing wraps
                ax, ay = inp.abs().amax(dim=1), y.abs().amax(dim=(1, 2, 3))
                big = (ay > 0) & (ax > torch.div(((1 << 62) - 1) // l.T, ay.clamp_min(1), rounding_mode="floor"))
                bad |= big
                a = torch.where(big[:, None, None, None], 0, a)
                # an int64 matmul does not exist on the GPU: a broadcast multiply and an integer sum over t
                out = (a[:, :, :, :, None] * y[:, :, None, :, :]).sum(dim=3).reshape(B, -1)
            elif isinstance(l, L.Concat):
                out = torch.cat([ctx[s + 1].reshape(B, -1) for s in l.srcs], dim=1)
            else:  # Flatten, Projection, BaseExtension: value-preserving
                out = inp.reshape(B, -1)
            ctx.append(out)
            cur = out
        bad |= (cur < -h).any(dim=1) | (cur >= M - h).any(dim=1)
        return (bad, cur) if want_out else bad

    def outputs(self, xs) -> np.ndarray:
        """The exact quantized plaintext outputs (Circuit.plain_q_eval with the CRT modulus) of a batch, by the
        same batched evaluation: the bench's verification oracle for many inputs."""
        xs = np.asarray(np.stack([np.asarray(x, dtype=np.int64).reshape(-1) for x in xs]))
        if not self.batched:
            return np.stack([self.circuit.plain_q_eval(x, False, self.M) for x in xs])
        import torch

        dev = self._tdev()
        with torch.no_grad():
            X = torch.as_tensor(xs).to(dev)
            outs = [self._bad_batch(X[k:k + self.CHUNK], True)[1] for k in range(0, len(xs), self.CHUNK)]
            return torch.cat(outs).cpu().numpy()

    # ------------------------------------------------------------------ native GPU path
    def native_spec(self) -> dict:
        """The DevRangeGuard description of the circuit. Elementwise layers (rescale, ReLU, sign, value-preserving)
        whose input is read by no other layer are fused into the epilogue of the layer before them ("post": each
        checks its input range, then applies its function); every remaining group is one launch. Activation
        buffers are shared by values whose lifetimes do not overlap."""
        c, M, h = self.circuit, self.M, _half(self.M)
        lay = c.layers
        n = len(lay)
        srcs = []
        for i, l in enumerate(lay):
            src = getattr(l, "in_src", None)
            srcs.append(src + 1 if src is not None else i)
        readers: dict = {}
        for i, l in enumerate(lay):
            readers.setdefault(srcs[i], []).append(i)
            if isinstance(l, L.Add):
                readers.setdefault(l.src + 1, []).append(i)
        elem = (L.Rescale, L.Relu, L.Sign, L.Flatten, L.Projection, L.BaseExtension)

        def op_of(i):
            l, d = lay[i], {}
            lim = self._limits(l)
            if lim is not None:
                d.update(check=True, lo=int(lim[0]), hi=int(lim[1]))
            if isinstance(l, L.Rescale):
                if l.use_sign_base_extension:
                    d.update(kind=2, l=int(l.l), c=int(h % 2))
                else:
                    S = int(np.prod(l.s))
                    d.update(kind=3, S=S, c=int(h % S))
            elif isinstance(l, L.Relu):
                d.update(kind=4)
            elif isinstance(l, L.Sign):
                d.update(kind=5)
            else:
                d.update(kind=9)
            return d

        # groups: a head layer and the elementwise layers fused after it
        groups, i = [], 0
        while i < n:
            g, j = [i], i + 1
            while (j < n and isinstance(lay[j], elem) and srcs[j] == j and readers.get(j) == [j]
                   and len(g) - (0 if isinstance(lay[i], elem) else 1) < 6):
                g.append(j)
                j += 1
            groups.append(g)
            i = j
        # buffers: the output of group k (context index g[-1] + 1) lives until the last group that reads it
        group_of_ctx = {g[-1] + 1: k for k, g in enumerate(groups)}
        last_use = {n: len(groups)}
        for k, g in enumerate(groups):
            ins = [srcs[g[0]]] + ([lay[g[0]].src + 1] if isinstance(lay[g[0]], L.Add) else [])
            for ci in ins:
                assert ci == 0 or ci in group_of_ctx, "range guard: a fused value is read by a later layer"
                last_use[ci] = max(last_use.get(ci, -1), k)
        ctx_buf, buf_elems, holder, layers = [0] * (n + 1), [], [], []
        for k, g in enumerate(groups):
            head = lay[g[0]]
            out_ctx = g[-1] + 1
            out_size = int(lay[g[-1]].out_size)
            free = [b for b, cj in enumerate(holder) if last_use.get(cj, -1) < k]
            if free:
                b = free[0]
                buf_elems[b] = max(buf_elems[b], out_size)
                holder[b] = out_ctx
            else:
                b = len(holder)
                holder.append(out_ctx)
                buf_elems.append(out_size)
            for j in g:
                ctx_buf[j + 1] = b
            d = dict(src=srcs[g[0]], buf=b, in_size=int(head.in_size), out_size=out_size)
            post = [op_of(j) for j in g[1:]]
            if isinstance(head, L.Conv2d):
                d.update(kind=0, C=head.C, H=head.H, W=head.W, F=head.F, kh=head.kh, kw=head.kw, sh=head.sh,
                         sw=head.sw, ph=head.ph, pw=head.pw, OH=head.OH, OW=head.OW, g=head.groups,
                         w=_i32(head.q_weights.reshape(head.F, -1)), b=np.asarray(head.q_biases, np.int64))
            elif isinstance(head, L.Dense):
                perm = None
                if head.channel_tf:
                    K, ch = head.in_size, head.channel_tf
                    kk = np.arange(K)
                    perm = (kk // ch + (kk % ch) * (K // ch)).astype(np.int32)
                d.update(kind=1, w=_i32(head.q_weights), b=np.asarray(head.q_biases, np.int64).reshape(-1), perm=perm)
            elif isinstance(head, (L.MaxPool2d, L.SumPool2d)):
                d.update(kind=6 if isinstance(head, L.MaxPool2d) else 7, C=head.C, H=head.H, W=head.W, kh=head.kh,
                         kw=head.kw, sh=head.sh, sw=head.sw, OH=head.OH, OW=head.OW, span_max=int(self.span_max()))
                lim = self._limits(head)
                if lim is not None:
                    d.update(check=True, lo=int(lim[0]), hi=int(lim[1]))
            elif isinstance(head, L.Add):
                d.update(kind=8, add_src=int(head.src + 1))
            else:  # an elementwise head: its own op first
                d.update(kind=9)
                post = [op_of(g[0])] + post
            d["post"] = post
            layers.append(d)
        return dict(layers=layers, input_size=int(c.input_size), ctx_buf=ctx_buf, buf_elems=buf_elems,
                    out_lo=-h, out_hi=M - h)

    def _native(self):
        if self._dev is None:
            from ..native import native

            spec = self.native_spec()
            per_input = 8 * sum(spec["buf_elems"])
            chunk = int(max(1, min(64, (256 << 20) // max(1, per_input))))
            self._dev = native().DevRangeGuard(int(self.device), spec["layers"], spec["input_size"], spec["ctx_buf"],
                                               spec["buf_elems"], spec["out_lo"], spec["out_hi"], chunk)
        return self._dev

    def _native_ok(self) -> bool:
        if self.device is None or not self.batched or not self.native_forms:
            return False
        try:
            import torch

            return torch.cuda.is_available()
        except ImportError:  # pragma: no cover
            return False

    # ------------------------------------------------------------------ public API
    def submit(self, xs) -> "PendingCheck":
        """Start the check of a batch of inputs; on a GPU it runs on its own stream (DevRangeGuard),
        overlapping the garbled evaluation launched before. ``PendingCheck.raise_if_bad()`` before releasing
        the results."""
        xs = np.asarray(np.stack([np.asarray(x, dtype=np.int64).reshape(-1) for x in xs]))
        if not self.batched:
            return PendingCheck(self, xs, None, None)
        if self._native_ok():
            g = self._native()
            return PendingCheck(self, xs, None, None, native=(g, g.submit(xs)))
        import torch

        dev = self._tdev()
        if dev.type == "cuda":
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=dev)
            st = self._stream
            st.wait_stream(torch.cuda.current_stream(dev))  # staging of an earlier submit is free again
            with torch.cuda.stream(st):
                X = torch.as_tensor(xs).pin_memory().to(dev, non_blocking=True)
                flags = torch.cat([self._bad_batch(X[k:k + self.CHUNK]) for k in range(0, len(xs), self.CHUNK)])
                host = flags.to("cpu", non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(st)
            return PendingCheck(self, xs, host, ev)
        with torch.no_grad():
            X = torch.as_tensor(xs)
            flags = torch.cat([self._bad_batch(X[k:k + self.CHUNK]) for k in range(0, len(xs), self.CHUNK)])
        return PendingCheck(self, xs, flags, None)

    def check(self, xs) -> None:
        self.submit(xs).raise_if_bad()


class PendingCheck:
    def __init__(self, guard: RangeGuard, xs: np.ndarray, flags, event, native=None):
        self.guard, self.xs, self.flags, self.event = guard, xs, flags, event
        self.native = native
        self._bad = None

    def bad_indices(self) -> List[int]:
        if self._bad is not None:
            return self._bad
        if self.native is not None:  # DevRangeGuard: bit 0 violation, bit 1 activations beyond int32 operands
            g, ticket = self.native
            f = np.asarray(g.wait(ticket))
            self.native = None
            # an uncertain input's device activations are not exact from the layer that marked it on, so its
            # bit 0 means nothing either way (a wrapped 24-bit sum can look like a violation): the host decides
            self._bad = [int(i) for i in np.nonzero(f == 1)[0]]
            self._bad += [int(i) for i in np.nonzero(f & 2)[0] if self.guard.violations_np(self.xs[i])]
            self._bad.sort()
            return self._bad
        if self.flags is None:  # per-input numpy path
            return [i for i, x in enumerate(self.xs) if self.guard.violations_np(x)]
        if self.event is not None:
            self.event.synchronize()
        return [int(i) for i in np.nonzero(self.flags.numpy())[0]]

    def raise_if_bad(self) -> None:
        bad = self.bad_indices()
        if bad:
            i = bad[0]
            v = self.guard.violations_np(self.xs[i])
            raise RangeGuardError(
                f"range guard: {len(bad)} of {len(self.xs)} input(s) would leave an exact gadget range (first: "
                f"input {i}, layer/lo/hi violations {v}); the garbled result would be a valid but wrong label. "
                f"Refused: use rescale='legacy' or a larger CRT base for such inputs")


def _i32(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.int64)
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError("range guard: weights beyond int32")
    return a.astype(np.int32)


def guard_for(circuit, crt_modulus: int, mrs: bool, device: Optional[int] = None,
              joint_clips: Optional[dict] = None) -> RangeGuard:
    """The circuit's cached guard (weights staged once per device)."""
    cache = circuit.__dict__.setdefault("_range_guards", {})
    key = (int(crt_modulus), bool(mrs), device, tuple(sorted((joint_clips or {}).items())))
    g = cache.get(key)
    if g is None:
        g = cache[key] = RangeGuard(circuit, crt_modulus, mrs, device, joint_clips)
    return g
