"""MI355X-native training step of the feed-forward acoustic model (BASELINE configs 1/2).

What the reference does per mini-batch in ModularModelHandlerPyTorch.process_dataloader
(:745-820) for an `RNNDYN-2_TANH_512-1_FC_187` model -- FFWrapper forward (FFWrapper.py:63-73),
NamedLoss masked MSE 'mean_per_frame' (NamedLoss.py:70-117), backward, Adam -- is done here on
*packed valid frames* (FF layers are frame independent, so padding is never computed) with all
parameters, gradients and Adam moments in ONE flat fp32 buffer each:

  fwd   3 x fp32-MFMA GEMM with fused bias+tanh
  loss  fused masked-MSE + dLoss/dPred
  bwd   dX GEMMs with the previous layer's tanh' fused in the epilogue, dW GEMMs with
        deterministic split-K slabs, bias column sums
  DP    one all-reduce(sum) of the flat gradient buffer over RCCL (torch.distributed 'nccl');
        local gradients are already divided by the GLOBAL valid-frame count, so the result equals
        the single-GPU step on the concatenated batch
  opt   one fused Adam launch over the flat buffers
"""
import math

import torch

from . import ops


def _pad4(n):
    return (n + 3) // 4 * 4


# Largest share of non-zeros in the first batch's input at which sparse_input=None takes the row-list path for
# layer 0's forward product.  From the density sweep at the bench shape in DESIGN.md section 21 (list build + sparse
# forward against the dense forward launch, kernel time): 0.69 of the dense time at 10 % non-zeros, 1.02 at 20 %,
# equal at 19 % by interpolation; the constant stays a little below that.
SPARSE_INPUT_MAX_DENSITY = 0.18

# The same for sparse_wgrad=None and layer 0's weight gradient, from the dW columns of the same sweep (column build +
# sparse launch against the dense launch): 0.85 of the dense time at 7 % non-zeros, 0.98 at 10 %, 1.34 at 20 %.  The
# column form crosses over much earlier than the forward's row form, so it has a constant of its own.
SPARSE_WGRAD_MAX_DENSITY = 0.09


class FlatFFModel:
    """Dense stack dims[0] -> dims[1] -> ... with activations `acts` (one per layer: a name of ops.ACT_BY_NAME in
    any case, e.g. "tanh" / "Sigmoid", an ops.ACT_* code, or None).

    sparse_input: True / False sends layer 0's forward product of a training step through the row lists of its
    input (ops.sparse_rows_build + ops.linear_fwd_sparse) / through the dense product.  None decides once, at the
    first loss_and_backward, from the density of that batch (one host synchronisation in the model's life) and keeps
    the decision: a later dense batch is slower on the sparse path, never wrong.

    sparse_wgrad: True / False sends layer 0's weight gradient through column lists of the same input
    (ops.sparse_cols_build + ops.linear_bwd_weight_sparse) / through the dense product; None takes the lists where
    sparse_input does and the first batch's density is at most SPARSE_WGRAD_MAX_DENSITY.  The column plan is made
    once, from the column counts of the first batch (read where the density decision is made), and is a hint for
    speed only.

    cols_from_lists: the column data of a step are made from the row lists that the step's sparse forward built from
    the same input (the same block as from the input itself, without a second pass over it); False restores the
    build from the input.

    dropouts: one probability in [0, 1) per layer (default: none) of the dropout behind the layer's activation, as
    `LayerConfig(dropout=...)` puts an nn.Dropout behind every layer of a Linear group.  A training step applies it
    in the epilogues of the products (csrc/dropout.h: the mask of an element follows from the step's seed, the layer
    and the element's position, so the backward recomputes it and none is stored); forward() without training=True,
    the validation and inference forward, is the model without dropout."""

    cols_from_lists = True

    def __init__(self, dims=(425, 512, 512, 187), acts=("tanh", "tanh", None), device="cuda",
                 seed=0, state_dict=None, sparse_input=None, sparse_wgrad=None, dropouts=None):
        assert len(acts) == len(dims) - 1
        self.dropouts = [0.0] * len(acts) if dropouts is None else [float(p) for p in dropouts]
        if len(self.dropouts) != len(acts) or not all(0.0 <= p < 1.0 for p in self.dropouts):
            raise ValueError("dropouts: one probability in [0, 1) per layer, got {!r}".format(dropouts))
        self.dims = tuple(int(d) for d in dims)
        self.acts = [ops.act_code(a) for a in acts]
        self.device = torch.device(device)
        # Row pitch of every weight matrix (and of the packed input) is padded to a multiple of
        # 4 floats so all GEMM operands take the 16-byte load path; pad columns stay exactly zero
        # (their gradient is dz^T * 0 = 0, Adam leaves a zero parameter with zero moments at zero).
        self.in_pitch = _pad4(self.dims[0])
        self.layout = []  # (w_off, b_off, N, K, Kpitch)
        off = 0
        for li, (K, N) in enumerate(zip(self.dims[:-1], self.dims[1:])):
            kp = _pad4(K) if li == 0 else K
            w_off = off
            off += _pad4(N * kp)
            b_off = off
            off += _pad4(N)
            self.layout.append((w_off, b_off, N, K, kp))
        self.numel = off
        self.params = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.step_count = 0
        self._buffers = {}
        self.sparse_input = None if sparse_input is None else bool(sparse_input)
        self._lists = None        # the row lists of the current batch: the model's own storage
        self.sparse_wgrad = None if sparse_wgrad is None else bool(sparse_wgrad)
        self._col_plan = None     # ops.SparseColsPlan of layer 0's input, made once
        self._cols = None         # the column data of the current batch: the model's own storage
        if state_dict is None:
            state_dict = self.reference_init(self.dims, seed)
        self.load_layers(state_dict)

    # torch.nn.Linear default init in the order the reference constructs the layers
    @staticmethod
    def reference_init(dims, seed):
        g = torch.Generator().manual_seed(seed)
        layers = []
        for K, N in zip(dims[:-1], dims[1:]):
            bound = 1.0 / math.sqrt(K)
            w = (torch.rand(N, K, generator=g) * 2 - 1) * bound
            b = (torch.rand(N, generator=g) * 2 - 1) * bound
            layers.append((w, b))
        return layers

    @staticmethod
    def from_module(model, device=None):
        """Mirror of a drop-in module stack (NamedForwardWrapper / RNNDyn) that consists of Linear
        groups only: same weights, flat buffers.  Returns None when the model has anything else
        (recurrent groups, Conv1d groups, LayerNorm groups, a dropout with p = 1 or in front of the first layer) --
        those train through the module path.  The nn.Dropout behind a layer becomes that layer's entry of
        `dropouts`."""
        from .nn.modules import LinearAct
        inner = getattr(model, "model", model)
        layers, acts, drops = [], [], []
        for group in getattr(inner, "layer_groups", []):
            seq = getattr(group, "module", None)
            if not isinstance(seq, torch.nn.Sequential):
                return None
            for m in seq:
                if isinstance(m, LinearAct):
                    layers.append((m.weight.detach(), m.bias.detach()))
                    acts.append(ops.ACT_TORCH_NAME.get(m.act))
                    drops.append(0.0)
                elif isinstance(m, torch.nn.Dropout):
                    if type(m).__name__ != "Dropout" or not layers or drops[-1] != 0.0 or not 0.0 <= m.p < 1.0:
                        return None
                    drops[-1] = float(m.p)
                elif isinstance(m, torch.nn.Conv1d):
                    return None
                elif type(m).__name__ != "FusedActivation":
                    return None
        if not layers:
            return None
        dims = [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers]
        device = device if device is not None else layers[0][0].device
        return FlatFFModel(dims, acts, device=device, state_dict=layers, dropouts=drops)

    def store_to_module(self, model, buf=None):
        """Writes the flat parameters (or another buffer of the same layout, e.g. the EMA shadow)
        back into the module stack (checkpoints, inference)."""
        from .nn.modules import LinearAct
        inner = getattr(model, "model", model)
        mods = [m for g in inner.layer_groups for m in g.module if isinstance(m, LinearAct)]
        with torch.no_grad():
            for i, m in enumerate(mods):
                m.weight.copy_(self.weight(i, buf))
                m.bias.copy_(self.bias(i, buf))
        return mods

    def load_layers(self, layers):
        for i, (w, b) in enumerate(layers):
            self.weight(i).copy_(w.to(self.device))
            self.bias(i).copy_(b.to(self.device))

    def weight_padded(self, i, buf=None):
        """[N, Kpitch] contiguous storage of layer i (pad columns are zero)."""
        w_off, _, N, K, kp = self.layout[i]
        return (self.params if buf is None else buf)[w_off:w_off + N * kp].view(N, kp)

    def weight(self, i, buf=None):
        """[N, K] view with the reference's state-dict shape (strided when K is padded)."""
        K = self.layout[i][3]
        return self.weight_padded(i, buf)[:, :K]

    def bias(self, i, buf=None):
        _, b_off, N, _, _ = self.layout[i]
        return (self.params if buf is None else buf)[b_off:b_off + N]

    def pack_input(self, x):
        """[M, dims[0]] -> [M, in_pitch] with zero pad columns (done once per batch at collate
        time; a loader can write into the padded buffer directly)."""
        if x.shape[1] == self.in_pitch:
            return x
        xp = torch.zeros((x.shape[0], self.in_pitch), dtype=torch.float32, device=x.device)
        xp[:, :x.shape[1]] = x
        return xp

    def layers(self):
        return [(self.weight(i).clone(), self.bias(i).clone()) for i in range(len(self.layout))]

    # ------------------------------------------------------------------------------------
    def _rows_buffer(self, name, M, width):
        """[M, width] view of a persistent zero-initialised buffer whose row pitch is padded to a
        multiple of 4 floats (16-byte GEMM loads); the pad columns are never written, so they
        stay zero.  One buffer per name, grown to the largest M seen."""
        pitch = _pad4(width)
        buf = self._buffers.get(name)
        if buf is None or buf.shape[0] < M:
            buf = torch.zeros((M, pitch), dtype=torch.float32, device=self.device)
            self._buffers[name] = buf
        return buf[:M, :width]

    def has_dropout(self):
        return any(p > 0.0 for p in self.dropouts)

    def forward(self, x, n_layers=None, sparse=False, training=False, seed=None):
        """x [M, dims[0]] fp32 packed frames -> list of layer outputs (of the first n_layers).  sparse: layer 0
        walks the row lists of x, built here, instead of the dense product.  training=True applies the layers'
        dropout with the masks of `seed` (an integer; layer i's salt is i): the outputs are the dropped ones."""
        acts = []
        h = self.pack_input(x)
        M = h.shape[0]
        if training and seed is None and self.has_dropout():
            raise ValueError("a training forward of a model with dropout needs a seed")
        for i in range(len(self.layout) if n_layers is None else n_layers):
            out = self._rows_buffer("h%d" % i, M, self.layout[i][2])
            p = self.dropouts[i] if training else 0.0
            drop = ops._drop_args(p, seed, i, 0) if p > 0.0 else None
            if i == 0 and sparse:
                self._lists = ops.sparse_rows_build(h, lists=self._lists, want_record=False)
                h = ops._linear_fwd_sparse(self._lists, h, self.weight_padded(i), self.bias(i), self.acts[i], out, drop)
            else:
                h = ops._linear_fwd(h, self.weight_padded(i), self.bias(i), self.acts[i], out, drop)
            acts.append(h)
        return acts

    def _decide_sparse_input(self, x):
        """sparse_input=None: the density of this (the first) batch against the measured crossover."""
        self._lists = ops.sparse_rows_build(x, lists=self._lists, want_record=True)
        self.sparse_input = self._lists.density() <= SPARSE_INPUT_MAX_DENSITY

    def _use_sparse_wgrad(self, x):
        """whether layer 0's weight gradient takes the column lists of x; the first call that says yes makes the
        plan (it reads the column counts of x: a synchronisation, at the same place as the density decision)"""
        fits = self.dims[0] <= ops.SPARSE_COLS_MAX_K
        if self.sparse_wgrad is None:
            self.sparse_wgrad = False
            if self.sparse_input and fits:
                plan = ops.sparse_cols_plan(x, K=self.dims[0])
                if plan.density <= SPARSE_WGRAD_MAX_DENSITY:
                    self.sparse_wgrad, self._col_plan = True, plan
        if not self.sparse_wgrad:
            return False
        if self._col_plan is None and fits:
            self._col_plan = ops.sparse_cols_plan(x, K=self.dims[0])
        return True

    def loss_and_backward(self, x, target, row_valid, n_valid_global, reduce_group=None, reduce=False, seed=None):
        """Fills self.grads with d(loss)/d(params) of this rank's frames; returns loss tensor
        (this rank's contribution, already divided by the global frame count).  reduce=True (data
        parallel): the sum all-reduce of a layer's gradient segment is issued as soon as its weight
        gradient is queued -- it runs on the collective's own stream under the remaining GEMMs --
        and the handles are left in self._pending for train_step to wait on before Adam.  seed: of this step's
        dropout masks (a model with dropouts); None draws one from the process's stream (nn.functional.DropoutStream:
        every rank of a data-parallel run its own)."""
        self._pending = []
        self._seed = 0
        if self.has_dropout():
            # (a training step captured into a graph would replay this seed, and with it one mask, on every replay;
            # nothing captures training steps)
            if seed is None:
                from .nn.functional import default_dropout_stream
                seed = default_dropout_stream().next()
            self._seed = int(seed)
        x = self.pack_input(x)
        if self.sparse_input is None:
            self._decide_sparse_input(x)
        self._wgrad_sparse_now = self._use_sparse_wgrad(x)
        if reduce:
            return self._loss_and_backward(x, target, row_valid, n_valid_global, reduce_group, reduce)
        # one process: the loss sum and the layers' split-K slab reductions are queued and run as ONE
        # launch at the end (five launches less per step); with data parallelism every layer's
        # gradient is reduced at once, because its all-reduce starts right behind it
        with ops.deferred_reductions():
            return self._loss_and_backward(x, target, row_valid, n_valid_global, reduce_group, False)

    def _loss_and_backward(self, x, target, row_valid, n_valid_global, reduce_group, reduce):
        M = x.shape[0]
        n = len(self.layout)
        drops, seed = self.dropouts, self._seed
        if drops[-1] > 0.0:
            # the output layer itself carries dropout: the fused output-layer + loss epilogue has no registers left
            # for the rule, so the layer stores its (dropped) output, the loss reads it, and its gradient goes back
            # through the dropout and the activation in one elementwise pass
            hs = self.forward(x, sparse=bool(self.sparse_input), training=True, seed=seed)
            loss, dz = ops.masked_mse(hs[-1], target, row_valid, n_valid_global,
                                      grad=self._rows_buffer("dz_out", M, self.dims[-1]))
            if self.acts[-1] in (None, ops.ACT_NONE):
                dz = ops.dropout_apply(dz, drops[-1], seed, n - 1, out=dz)
            else:
                dz = ops.dropout_act_bwd(dz, hs[-1], self.acts[-1], drops[-1], seed, n - 1, out=dz)
        elif self.acts[-1] in (None, ops.ACT_NONE) and n > 1:
            # the output layer never materialises: its GEMM epilogue forms the masked difference
            # to the target, the loss partial sums and d loss / d output
            hs = self.forward(x, n_layers=n - 1, sparse=bool(self.sparse_input), training=True, seed=seed)
            loss, dz = ops.linear_fwd_mse(hs[-1], self.weight_padded(n - 1), self.bias(n - 1), target,
                                          row_valid, n_valid_global,
                                          grad=self._rows_buffer("dz_out", M, self.dims[-1]))
            hs.append(None)
        else:
            hs = self.forward(x, sparse=bool(self.sparse_input), training=True, seed=seed)
            loss, dz = ops.masked_mse(hs[-1], target, row_valid, n_valid_global,
                                      grad=self._rows_buffer("dz_out", M, self.dims[-1]))
            if self.acts[-1] != ops.ACT_NONE:
                # d loss / d output -> d loss / d pre-activation of the output layer (the loop below starts there)
                dz = ops.act_bwd(dz, hs[-1], self.acts[-1])
        for i in range(n - 1, -1, -1):
            inp = hs[i - 1] if i > 0 else x
            dz_in = None
            if i > 0:
                # dW, db and the input gradient of the layer in one call (one launch)
                dz_in = self._rows_buffer("dz%d" % (i & 1), M, self.layout[i][3])
                drop = ops._drop_args(drops[i - 1], seed, i - 1, 0) if drops[i - 1] > 0.0 else None
                ops._linear_bwd(dz, inp, self.weight_padded(i), self.weight_padded(i, self.grads),
                                self.bias(i, self.grads), dz_in, hs[i - 1], self.acts[i - 1], False, drop)
            elif self._wgrad_sparse_now:
                # without a plan (dims[0] > 512) the entry point runs the dense product and counts it
                if self._col_plan is not None:
                    # the forward above listed the non-zeros of this x when it took the sparse path
                    lists = self._lists if self.cols_from_lists and self.sparse_input else None
                    self._cols = ops.sparse_cols_build(x, self._col_plan, K=self.dims[0], cols=self._cols,
                                                       lists=lists)
                ops.linear_bwd_weight_sparse(dz, x, self._cols if self._col_plan is not None else None,
                                             self._col_plan, dw=self.weight_padded(i, self.grads),
                                             db=self.bias(i, self.grads), K=self.dims[0])
            else:
                ops.linear_bwd_weight(dz, inp, dw=self.weight_padded(i, self.grads),
                                      db=self.bias(i, self.grads))
            if reduce:
                from .parallel import allreduce_flat_
                w_off, b_off, N, _, _ = self.layout[i]
                work = allreduce_flat_(self.grads[w_off:b_off + _pad4(N)], reduce_group, async_op=True)
                if work is not None:
                    self._pending.append(work)
            if i > 0:
                dz = dz_in
        return loss

    def train_step(self, x, target, row_valid, n_valid_global, lr=1e-3, betas=(0.9, 0.999),
                   eps=1e-8, weight_decay=0.0, process_group=None, world_size=1,
                   clip_norm_kind=None, clip_max_norm=0.0, clip_value=None, ema_shadow=None,
                   ema_decay=0.0, seed=None):
        """forward + masked MSE + backward + [all-reduce] + optimiser tail.  clip_norm_kind 2 / 0
        (infinity) clips the gradient norm to clip_max_norm, clip_value clamps the elements,
        ema_shadow (flat, this model's layout) is updated with ema_decay -- all inside the one
        Adam pass (itts_adam_step_fused)."""
        from . import parallel
        dist_on = world_size > 1 or parallel._active(process_group)
        loss = self.loss_and_backward(x, target, row_valid, n_valid_global, reduce_group=process_group,
                                      reduce=dist_on, seed=seed)
        for work in self._pending:   # the optimiser's stream waits for the collectives
            work.wait()
        self._pending = []
        self.step_count += 1
        if clip_norm_kind is None and not clip_value and ema_shadow is None:
            ops.adam_step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, self.step_count,
                          lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
            return loss
        accum = None
        if clip_norm_kind is not None:
            if getattr(self, "_norm_accum", None) is None:
                self._norm_accum = torch.zeros(1, dtype=torch.float32, device=self.device)
            accum = ops.grad_norm_accum(self.grads, self._norm_accum, clip_norm_kind)
        ops.adam_step_fused(self.params, self.grads, self.exp_avg, self.exp_avg_sq,
                            self.step_count, lr=lr, betas=betas, eps=eps,
                            weight_decay=weight_decay, norm_accum=accum,
                            norm_kind=clip_norm_kind if clip_norm_kind is not None else 2,
                            clip_max_norm=clip_max_norm, clip_value=clip_value or 0.0,
                            ema_shadow=ema_shadow, ema_decay=ema_decay)
        return loss


def flops_per_frame(dims, skip_first_dgrad=True):
    """fwd + bwd FLOPs per valid frame: 2*N*K fwd, 2*N*K dW, 2*N*K dX (not for layer 0)."""
    f = 0
    for i, (K, N) in enumerate(zip(dims[:-1], dims[1:])):
        f += 2 * N * K * (2 if (i == 0 and skip_first_dgrad) else 3)
    return f
