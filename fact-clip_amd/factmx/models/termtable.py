"""The device term table of fx_loss_terms_fwd / fx_loss_terms_bwd, assembled in one place for every loss
phase (models/vloss.py, models/vn_vloss.py): the upload pack, the gradient arena, the per-term scratch
layout, the plan and the autograd node.  Nothing here knows a model; everything up to ``TermTable.send``
runs on plain CPU tensors without the native library, so the layout can be checked without a device."""
import ctypes

import numpy as np
import torch

from .. import native as nx


class _Pack:
    """Host tables and ABI structs laid out in one buffer: allocated on the device first (so the
    structs can hold device addresses), then filled on the host and sent by ONE non-blocking copy
    from pinned memory."""

    def __init__(self):
        self.items = []
        self.size = 0

    def _reserve(self, nbytes):
        off = (self.size + 15) & ~15
        self.size = off + max(int(nbytes), 4)
        return off

    def array(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        off = self._reserve(a.nbytes)
        self.items.append((off, a))
        return off

    def structs(self, ctype, n):
        arr = (ctype * n)()
        off = self._reserve(ctypes.sizeof(arr))
        self.items.append((off, arr))
        return off, arr

    def alloc(self, dev):
        self.dev = torch.empty(self.size, dtype=torch.uint8, device=dev)
        self.base = self.dev.data_ptr()
        return self.base

    def send(self):
        host = torch.empty(self.size, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        for off, a in self.items:
            b = np.frombuffer(a, dtype=np.uint8) if isinstance(a, ctypes.Array) else a.view(np.uint8)
            hv[off:off + b.size] = b
        self.dev.copy_(host, non_blocking=True)


def _contig_strides(shape):
    st, acc = [], 1
    for n in reversed(tuple(shape)):
        st.append(acc)
        acc *= int(n)
    return tuple(reversed(st))


class _LossFn(torch.autograd.Function):
    """(out, loss) = fx_loss_terms_fwd(term table): out = the coefficient matrix's rows (vloss.run: [batch
    loss, per video (loss, fact, contrastive, per-block)]), loss = out[0] as its own 0-dim output (the step's
    loss.backward() then enters this node directly: no select node, whose backward would zero-fill an nout
    vector and copy the scalar into it); backward writes every input's gradient whole."""

    @staticmethod
    def forward(ctx, plan, *inputs):
        lib = nx.load()
        dev = inputs[0].device
        out = torch.empty(plan["nout"], device=dev, dtype=torch.float32)
        nx.check(lib.fx_loss_terms_fwd(ctypes.addressof(plan["terms_host"]), plan["terms_dev"], plan["nterms"],
                                       plan["coef_dev"], plan["nout"], nx.ptr(out), nx.ptr(plan["ws"]), nx.stream()),
                 "fx_loss_terms_fwd")
        loss = out[0].clone()
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        return out, loss

    @staticmethod
    def backward(ctx, gout, gloss):
        plan = ctx.plan
        lib = nx.load()
        nout = plan["nout"]
        gflat, goff, shapes = plan["grads"]
        if gout is None and gloss is None:
            return (None,) + tuple(None for _ in shapes)
        if gout is None:           # only the batch loss was differentiated: row 0 of the coefficients alone
            gout, nout = gloss.reshape(1).contiguous(), 1
        else:
            gout = gout.contiguous()
            if gloss is not None:
                gout = gout.clone()
                gout[0] += gloss
        nx.check(lib.fx_loss_terms_bwd(ctypes.addressof(plan["terms_host"]), plan["terms_dev"], plan["nterms"],
                                       plan["coef_dev"], nout, nx.ptr(gout), nx.ptr(plan["ws"]), nx.stream()),
                 "fx_loss_terms_bwd")
        rb = plan.get("readback")
        if rb is not None and not rb.done:       # the step's read-back resolves when the backward pass ends
            torch.autograd.Variable._execution_engine.queue_callback(rb.resolve)
        # every input's gradient: its slice of the flat buffer, laid out as the input (contiguous)
        return (None,) + tuple(gflat.as_strided(shp, st, o) for o, (shp, st) in zip(goff, shapes))


class TermTable:
    """One term table on a ``_Pack`` the caller started (its label / target arrays are reserved already).

    The constructor reserves the coefficient matrix, the ``LossTerm`` array and ``nvn`` ``VnTerm`` structs,
    allocates the pack on ``dev`` and the gradient arena: ONE flat allocation, a 256-byte-aligned slice per
    differentiated input (``inputs`` de-duplicated by identity, first seen first), which the backward hands
    out as ``gflat.as_strided(shape, strides, offset)``.  ``add`` fills the next term (the caller's order is
    the kernels' summation order), ``lay_out`` places the scratch slots; ``coef`` and ``terms`` stay writable
    until ``send``; ``launch`` allocates the workspace, forms the plan and runs the forward."""

    def __init__(self, pk, dev, inputs, coef, nvn=0):
        self.pk, self.dev = pk, dev
        self.inputs, self._go, n = [], {}, 0
        for t in inputs:
            if id(t) not in self._go:
                self._go[id(t)] = n
                self.inputs.append(t)
                n += (t.numel() + 63) & ~63               # 256-byte aligned slices
        self.gflat = torch.empty(n, device=dev, dtype=torch.float32)
        self._gb = self.gflat.data_ptr()
        self.nout, self.nterms = coef.shape
        self._o_coef = pk.array(coef, np.float32)
        self.coef = pk.items[-1][1].reshape(coef.shape)    # (the buffer the pack sends)
        self._o_vn, self.vnt = pk.structs(nx.VnTerm, nvn) if nvn else (0, None)
        self._o_t, self.terms = pk.structs(nx.LossTerm, self.nterms)
        self.base = pk.alloc(dev)
        self._slots = []                                  # scratch sizes (lse, lse2, colz) per term
        self._keep = []
        self.scr = self.plan = None

    def grads(self):
        """Per input its gradient's element offset in ``gflat`` and its (shape, strides): the plan's ``grads``."""
        return [self._go[id(t)] for t in self.inputs], [(t.shape, _contig_strides(t.shape)) for t in self.inputs]

    def grad_ptr(self, t, off=0):
        """The address of element ``off`` of input ``t``'s gradient slice."""
        return self._gb + 4 * (self._go[id(t)] + off)

    def grad_slice(self, t):
        return self.gflat.narrow(0, self._go[id(t)], t.numel())

    def add(self, kind, R, C, x, sr, sc, g, goff, dsr, dsc, c_ce, c_sm, kcap=0, ncolz=0):
        """The next term: ``R`` x ``C`` logits at address ``x`` with element strides ``sr`` / ``sc``, their
        gradient at element ``goff`` of input ``g``'s slice with strides ``dsr`` / ``dsc`` (``g`` None: the
        caller sets ``dx``).  ``kcap``: the most matched columns an ATTN term will get (its ``K`` may be set
        later), ``ncolz``: an InfoNCE term's column scratch.  Returns the struct (``slot`` is its index) for
        the kind's own fields."""
        i = len(self._slots)
        t = self.terms[i]
        t.slot, t.kind, t.R, t.C, t.x, t.sr, t.sc = i, kind, R, C, x, sr, sc
        if g is not None:
            t.dx = self._gb + 4 * (self._go[id(g)] + goff)
        t.dsr, t.dsc, t.c_ce, t.c_sm = dsr, dsc, c_ce, c_sm
        self._slots.append((2 * R, 0, 0) if kind == nx.TERM_VNCLASS else (R, R + kcap, kcap) if kind == nx.TERM_ATTN
                           else (R, C, ncolz) if kind == nx.TERM_INFONCE else (R, 0, 0))
        return t

    def vn(self, j, vnmap, null):
        """Fills ``VnTerm`` j for heads of ``num_verbs + null`` / ``num_nouns + null`` columns; returns its
        (device address, host address) for a VNCLASS term's ``vn`` / ``vn_host``."""
        n1, n2 = vnmap.num_verbs + null, vnmap.num_nouns + null
        m = self.vnt[j]
        m.n1, m.n2, m.A, m.null = n1, n2, vnmap.num_actions, null
        tabs = vnmap.tables(self.dev) + vnmap.csr(self.dev, n1, n2)
        m.vids, m.nids, m.voff, m.vlist, m.noff, m.nlist = (t.data_ptr() for t in tabs)
        self._keep.append(tabs)
        return self.base + self._o_vn + j * ctypes.sizeof(nx.VnTerm), ctypes.addressof(m)

    def vn_pair(self, vnmap):
        """A model's two mappings: [frame / segment heads (V, N), token heads with the null column]."""
        return [self.vn(0, vnmap, 0), self.vn(1, vnmap, 1)]

    def lay_out(self):
        """Per-term scratch in one allocation: 16-byte-aligned lse, lse2, colz slots."""
        assert len(self._slots) == self.nterms, (len(self._slots), self.nterms)
        offs, n = [], 0
        for sz in self._slots:
            for m in sz:
                offs.append(n)
                n += (max(m, 1) + 3) & ~3
        self.scr = torch.empty(max(n, 1), device=self.dev, dtype=torch.float32)
        sb = self.scr.data_ptr()
        for i in range(self.nterms):
            t = self.terms[i]
            t.lse, t.lse2, t.colz = sb + 4 * offs[3 * i], sb + 4 * offs[3 * i + 1], sb + 4 * offs[3 * i + 2]

    def send(self):
        assert self.scr is not None, "lay_out() before send()"
        self.pk.send()

    def launch(self, keep=()):
        """After ``send``: the workspace, the plan (``keep``: whatever else the backward reads) and the
        forward.  Returns ``_LossFn.apply``'s (out, loss)."""
        ws = torch.empty(max(nx.load().fx_loss_terms_workspace_floats(self.nterms), 1), device=self.dev,
                         dtype=torch.float32)
        self.plan = dict(terms_host=self.terms, terms_dev=self.base + self._o_t, nterms=self.nterms,
                         coef_dev=self.base + self._o_coef, nout=self.nout, ws=ws, grads=(self.gflat,) + self.grads(),
                         keep=(self.pk, self.scr, self._keep, self.inputs, keep))
        return _LossFn.apply(self.plan, *self.inputs)
