"""MX (block-scaled) linears of the DiTs: the MXFP8 / MXFP6 switch, its state and the routing of a block's large linears.

MXFP8 (`fino_quantize_mxfp8` + `fino_gemm_mxfp8`): OCP e4m3 elements with one e8m0 scale per 32 K-elements, fp32 accumulate.
MXFP6 (`fino_quantize_mxfp6` + `fino_gemm_mxfp6`): OCP e2m3 -- e4m3's three mantissa bits, the block scale supplies the range --
with the same scales, at the FP4 matrix rate; with `rotate=True` every MX block of both operands is rotated by the 32-point
Walsh-Hadamard matrix first (`fino_quantize_mxfp6_rot`), which keeps the product and spreads outliers over their block.
Weights are quantised once when the switch is turned on, activations per call.
Attention, norms, modulation, embeddings and the output head stay in the model dtype.  There is no reference counterpart (SURVEY
F11): the result is compared with the model's own bf16 forward (tests/test_mxfp8_gpu.py, tests/test_mxfp6_gpu.py).
"""
import os


class MXLinearsMixin:
    """enable_mxfp8_linears / enable_mxfp6_linears for a model that names its MX weights in `_mx_linear_weights(pk)` (yielding
    `(layer, key, weight)` from the packed weights `pk`), keeps its kernel front end in `self.ops`, calls `_mx_invalidate()`
    from `reset_caches` and `_mx_requantise_if_pending()` from `forward`, and runs those linears through `_lin`."""
    _fp8 = {}             # (layer, key) -> (element bytes, MX scales) of that weight (this shared default is never written to)
    _fp8_pending = False  # MX was on when the parameters last moved / changed: re-quantise at the next forward
    _mx_fmt = 8           # element format of the `_fp8` entries: 8 = e4m3 (enable_mxfp8_linears), 6 = e2m3 (enable_mxfp6_linears)
    _mx_rotate = False    # MXFP6 only: block-Hadamard rotation of both operands (enable_mxfp6_linears(rotate=True))

    def enable_mxfp8_linears(self, enabled=True):
        """Run the model's large linears (see its class docstring) on the MXFP8 path.  The LayerNorm in front of a linear and
        the FFN's GELU emit MXFP8 activations directly (`_ln_q`, `_ffn_mxfp8`).  There is no `rotate=` here: e4m3's four
        exponent bits already absorb a block's outliers and the rotation of `enable_mxfp6_linears` gains it nothing measurable
        (GEMM rel-RMS 0.0375 -> 0.0373 on outlier channels)."""
        return self._enable_mx_linears(8, enabled)

    def enable_mxfp6_linears(self, enabled=True, rotate=False):
        """The same linears on the MXFP6 path.  Activations are quantised from the model dtype (no fused producers: LayerNorm
        and the FFN's GELU write the model dtype and `fino_quantize_mxfp6` follows).  One reduced precision at a time: raises
        ValueError while `enable_mxfp8_linears()` is on.  Independent of `enable_fp8_attention()` and `enable_cache()`;
        `enable_mxfp6_linears(False)` returns the model to its model-dtype output bit for bit.
        rotate: every 32-element MX block of the weights and of the activations is rotated by the Walsh-Hadamard matrix before
        it is quantised (`fino_quantize_mxfp6_rot`; exact algebra, the GEMM is unchanged): an outlier no longer sets the
        scale of its block alone, which brings e2m3 back to MXFP8-class error on operands with outlier channels or heavy tails.
        Calling again with another `rotate` while on re-quantises the weights."""
        return self._enable_mx_linears(6, enabled, bool(rotate))

    @property
    def mxfp6_rotate(self):
        """whether the MXFP6 linears are on with the block-Hadamard rotation"""
        return self._mx_on and self._mx_fmt == 6 and self._mx_rotate

    @property
    def _mx_on(self):
        """on, or on and waiting for the next forward to re-quantise"""
        return bool(self._fp8) or self._fp8_pending

    def _enable_mx_linears(self, fmt, enabled, rotate=False):
        if self._mx_on and self._mx_fmt != fmt:
            if not enabled:
                return self                                     # the other precision's switch: nothing of this one to drop
            raise ValueError(f"enable_mxfp{fmt}_linears: enable_mxfp{self._mx_fmt}_linears() is on -- one reduced precision at a "
                             f"time; call enable_mxfp{self._mx_fmt}_linears(False) first")
        self._fp8 = {}
        self._fp8_pending = False
        self._mx_rotate = False
        if not enabled:
            return self
        self._mx_fmt = fmt
        self._mx_rotate = rotate
        quantize = self._mx_quantize()
        for li, key, w in self._mx_linear_weights(self._packed or self._pack()):
            self._fp8[(li, key)] = quantize(w.detach().contiguous())
        return self

    def _mx_quantize(self):
        """the weight quantiser of the format that is on"""
        if self._mx_fmt != 6:
            return self.ops.quantize_mxfp8
        if self._mx_rotate:                                     # (the keyword only when on: the unrotated calls stay as they were)
            return lambda w: self.ops.quantize_mxfp6(w, rotate="weight")
        return self.ops.quantize_mxfp6

    def _mx_invalidate(self):
        """The parameters may have changed or moved: drop the quantised weights.  They are re-quantised lazily, by the next
        forward, from wherever the parameters are then: a `.to("cpu")` / `.float()` in between must not run the GPU quantiser on
        host tensors or leave the module half moved.  Returns whether MX was on."""
        was_on = self._mx_on
        self._fp8 = {}
        self._fp8_pending = was_on
        return was_on

    def _mx_requantise_if_pending(self):
        if self._fp8_pending:
            self._enable_mx_linears(self._mx_fmt, True, self._mx_rotate)

    def _ln_q(self, li, key, mode, x, **ln):
        """the LayerNorm in front of linear (li, key) emitted directly as that linear's MXFP8 activations (fino_ln_mxfp8: one
        pass instead of norm -> bf16 -> quantise), or None when the linear is not on the MXFP8 path"""
        o = self.ops
        if not self._fp8 or (li, key) not in self._fp8 or not hasattr(o, "ln_mxfp8") or os.environ.get("FINO_NO_LN_MXFP8"):
            return None                                         # (the environment variable: A/B knob, two passes)
        if self._mx_fmt == 6:
            return None                                         # MXFP6 takes the two-pass route: norm -> model dtype -> quantise
        return o.ln_mxfp8(mode, x, **ln)

    def _lin(self, li, key, x, w, b, epi=0, xq=None, **kw):
        """one of a block's large linears: MX when enabled (and K is a multiple of 128), else the model-dtype GEMM.
        xq: the activations already quantised (_ln_q); MXFP6 quantises `x` itself.
        keep (residual epilogues): a [rows, N] buffer that also receives y = T(acc + bias), the linear's own output"""
        wq = self._fp8.get((li, key)) if self._fp8 else None
        o = self.ops
        keep = kw.pop("keep", None)
        if wq is None and self._fp8 and key in ("kv", "q"):
            # token shards project K|V and Q separately: quantise those row blocks of the fused weight on first use
            # (MX scales are per output row, so this equals slicing the quantised fused weight)
            wq = self._fp8[(li, key)] = self._mx_quantize()(w.detach().contiguous())
        if wq is None:
            if keep is not None:
                kw["keep"] = keep                               # the GEMM's epilogue keeps y beside the residual result
            return o.gemm(x, w, b, epi, **kw)
        kw.pop("tile_m", None)                                  # (the MX GEMMs have one tile height)
        if self._mx_fmt == 6:
            mx_gemm, (xq, xs) = o.gemm_mxfp6, (o.quantize_mxfp6(x, rotate="act") if self._mx_rotate else o.quantize_mxfp6(x))
        else:
            mx_gemm, (xq, xs) = o.gemm_mxfp8, (xq if xq is not None else o.quantize_mxfp8(x))
        if keep is not None:
            kw["keep"] = keep                                   # one launch: fino_gemm_mxfp8_keep / fino_gemm_mxfp6_keep
        return mx_gemm(xq, xs, wq[0], wq[1], b, epi, **kw)

    def _ffn_mxfp8(self, li, x, xq, b1, b2, epi, **kw):
        """The FFN of block `li` as one MXFP8 pair: the up-projection's GELU epilogue emits the hidden activations already
        quantised and the down-projection (epilogue `epi`, its operands in `kw`) consumes them -- no bf16 round trip.  `xq`: the
        input already quantised (_ln_q), else `x` is.  None when either weight is not on the MX path or the format is MXFP6:
        the caller then runs the two linears through `_lin`."""
        w1q, w2q = self._fp8.get((li, "ff1")), self._fp8.get((li, "ff2"))
        if w1q is None or w2q is None or self._mx_fmt != 8:
            return None
        o = self.ops
        hq = o.gemm_mxfp8_q(*(xq if xq is not None else o.quantize_mxfp8(x)), w1q[0], w1q[1], b1, o.EPI_GELU_TANH)
        return o.gemm_mxfp8(hq[0], hq[1], w2q[0], w2q[1], b2, epi, **kw)
