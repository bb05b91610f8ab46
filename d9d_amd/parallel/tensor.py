"""Tensor parallelism (TP) + sequence parallelism (SP).

The reference DECLARES tp but rejects tp > 1
(d9d/module/parallelism/model/qwen3_moe.py:35-36); this is a real
implementation: colwise/rowwise DTensor sharding of attention and FFN
projections over the `tp` mesh dim with the boundary collectives on RCCL.

Forward math per block:
  x -> [copy-to-tp: fwd identity / bwd all-reduce]
    -> colwise projections (weight Shard(0), local out features)
    -> ... local-head attention or local-intermediate FFN ...
    -> rowwise projection (weight Shard(1), partial out)
    -> [fwd all-reduce / bwd identity] -> y

Sequence-parallel variant replaces the boundary collectives by
all-gather(seq) on entry and reduce-scatter(seq) on exit, so the
norm/residual region holds only S/tp of the sequence.
"""

import torch
import torch.distributed as dist
from torch import nn
from torch.distributed.device_mesh import DeviceMesh
from torch.distributed.tensor import DTensor, Placement, Replicate, Shard

from ..module.block.attention import GroupedQueryAttention
from ..module.block.ffn import SwiGLU
from .style import _to_local_class


class _CopyToTP(torch.autograd.Function):
    """fwd identity; bwd all-reduce (input used by all tp ranks)."""

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        return x

    @staticmethod
    def backward(ctx, grad):
        grad = grad.contiguous()
        dist.all_reduce(grad, group=ctx.group)
        return grad, None


class _SumGradFromTP(torch.autograd.Function):
    """fwd identity; bwd all-reduce — for params replicated inside the tp
    region (e.g. q/k norm weights) whose per-microbatch grads are partial."""

    @staticmethod
    def forward(ctx, w, group):
        ctx.group = group
        return w.view_as(w)

    @staticmethod
    def backward(ctx, grad):
        grad = grad.contiguous()
        dist.all_reduce(grad, group=ctx.group)
        return grad, None


_SUMGRAD_CLASS_CACHE: dict[tuple, type] = {}


def _install_tp_sumgrad(module: nn.Module, param_names: tuple[str, ...], group) -> None:
    """Swap `module`'s class so each named param reads through
    `_SumGradFromTP` during grad-enabled forward (identity otherwise)."""
    module._d9d_tp_group = group

    def _make_getter(name: str):
        def getter(self):
            p = self._parameters.get(name)
            if p is None:
                raise AttributeError(name)
            if torch.is_grad_enabled() and p.requires_grad:
                return _SumGradFromTP.apply(p, self._d9d_tp_group)
            return p

        return property(getter)

    key = (type(module), param_names)
    if key not in _SUMGRAD_CLASS_CACHE:
        ns = {name: _make_getter(name) for name in param_names}
        ns["_d9d_tp_sumgrad_params"] = param_names
        _SUMGRAD_CLASS_CACHE[key] = type(
            f"TPSumGrad{type(module).__name__}", (type(module),), ns
        )
    module.__class__ = _SUMGRAD_CLASS_CACHE[key]


class _ReduceFromTP(torch.autograd.Function):
    """fwd all-reduce (partial rowwise outputs); bwd identity."""

    @staticmethod
    def forward(ctx, x, group):
        x = x.contiguous()
        dist.all_reduce(x, group=group)
        return x

    @staticmethod
    def backward(ctx, grad):
        return grad, None


class _AllGatherSeq(torch.autograd.Function):
    """fwd all-gather along dim; bwd reduce-scatter (SP entry)."""

    @staticmethod
    def forward(ctx, x, group, dim):
        ctx.group = group
        ctx.dim = dim
        world = dist.get_world_size(group)
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x.contiguous(), group=group)
        return torch.cat(parts, dim=dim)

    @staticmethod
    def backward(ctx, grad):
        return _reduce_scatter_dim(grad, ctx.group, ctx.dim), None, None


def _reduce_scatter_dim(x: torch.Tensor, group, dim: int) -> torch.Tensor:
    """Sum across ranks, return this rank's chunk along `dim`.

    RCCL path: reduce_scatter_tensor (ring over xGMI). gloo's list-based
    reduce_scatter mis-reduces interleaved chunks, so the CPU path does
    all-reduce + slice.
    """
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    x = x.contiguous()
    if x.is_cuda and dim == 0:
        out = torch.empty_like(x.chunk(world, dim=0)[0])
        dist.reduce_scatter_tensor(out, x, group=group)
        return out
    if x.is_cuda:
        moved = x.movedim(dim, 0).contiguous()
        out = torch.empty_like(moved.chunk(world, dim=0)[0])
        dist.reduce_scatter_tensor(out, moved, group=group)
        return out.movedim(0, dim).contiguous()
    dist.all_reduce(x, group=group)
    return x.chunk(world, dim=dim)[rank].contiguous()


class _AllGatherSeqSliceBwd(torch.autograd.Function):
    """fwd all-gather along dim; bwd SLICE own shard (no sum) — for consumers
    whose backward already all-reduces the grad over the group (the
    vocab-parallel CCE head reduces de internally, so a reduce-scatter here
    would double it)."""

    @staticmethod
    def forward(ctx, x, group, dim):
        ctx.group = group
        ctx.dim = dim
        world = dist.get_world_size(group)
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x.contiguous(), group=group)
        return torch.cat(parts, dim=dim)

    @staticmethod
    def backward(ctx, grad):
        world = dist.get_world_size(ctx.group)
        rank = dist.get_rank(ctx.group)
        return grad.chunk(world, dim=ctx.dim)[rank].contiguous(), None, None


class _ReduceScatterSeq(torch.autograd.Function):
    """fwd reduce-scatter along dim; bwd all-gather (SP exit)."""

    @staticmethod
    def forward(ctx, x, group, dim):
        ctx.group = group
        ctx.dim = dim
        return _reduce_scatter_dim(x, group, dim)

    @staticmethod
    def backward(ctx, grad):
        world = dist.get_world_size(ctx.group)
        parts = [torch.empty_like(grad) for _ in range(world)]
        dist.all_gather(parts, grad.contiguous(), group=ctx.group)
        return torch.cat(parts, dim=ctx.dim), None, None


def _shard_linear(lin: nn.Linear, mesh: DeviceMesh, tp_dim: int, shard_dim: int) -> None:
    """Replace lin.weight with its LOCAL shard wrapped as a DTensor.

    shard_dim 0 = colwise (split out features); 1 = rowwise (split in features).
    """
    tp_size = mesh.shape[tp_dim]
    tp_rank = mesh.get_coordinate()[tp_dim]
    w = lin._parameters["weight"]
    full = w.data
    local = full.chunk(tp_size, dim=shard_dim)[tp_rank].contiguous()
    placements: list[Placement] = [Replicate()] * mesh.ndim
    placements[tp_dim] = Shard(shard_dim)
    dt = DTensor.from_local(local, mesh, tuple(placements), run_check=False)
    lin._parameters["weight"] = nn.Parameter(dt, requires_grad=w.requires_grad)
    if shard_dim == 0:
        lin.out_features = local.shape[0]
        b = lin._parameters.get("bias")
        if b is not None:
            tp_rank = mesh.get_coordinate()[tp_dim]
            local_b = b.data.chunk(tp_size, dim=0)[tp_rank].contiguous()
            bp: list[Placement] = [Replicate()] * mesh.ndim
            bp[tp_dim] = Shard(0)
            lin._parameters["bias"] = nn.Parameter(
                DTensor.from_local(local_b, mesh, tuple(bp), run_check=False),
                requires_grad=b.requires_grad,
            )
    else:
        lin.in_features = local.shape[1]
    if not getattr(lin, "_d9d_to_local_params", None):
        names = ("weight", "bias") if lin._parameters.get("bias") is not None else ("weight",)
        lin.__class__ = _to_local_class(type(lin), names)


def parallelize_tp_attention(
    attn: GroupedQueryAttention, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    assert attn.num_heads % tp_size == 0 and attn.num_kv_heads % tp_size == 0, (
        "attention heads must divide tp"
    )
    _shard_linear(attn.q_proj, mesh, tp_dim, 0)
    _shard_linear(attn.k_proj, mesh, tp_dim, 0)
    _shard_linear(attn.v_proj, mesh, tp_dim, 0)
    _shard_linear(attn.o_proj, mesh, tp_dim, 1)
    attn.num_heads //= tp_size
    attn.num_kv_heads //= tp_size

    # Replicated params INSIDE the tp region see only the local heads'
    # activations, so their gradients are partial: sum them over tp.
    # (q_norm/k_norm weights are shared across heads; learnable sinks are
    # per-head and follow the q-head shard instead.)
    #
    # The reduction lives IN the autograd graph (`_SumGradFromTP` wraps the
    # weight each forward), so each microbatch's partial grad is reduced
    # exactly once before it accumulates into .grad — a post-accumulate hook
    # would re-reduce earlier microbatches' already-summed contributions
    # under gradient accumulation.
    for norm in (attn.q_norm, attn.k_norm):
        if norm is not None:
            _install_tp_sumgrad(norm, ("weight",), group)
    if attn.sinks is not None:
        rank = dist.get_rank(group)
        shard = attn.sinks.shape[0] // tp_size
        with torch.no_grad():
            local_sinks = attn.sinks[rank * shard : (rank + 1) * shard].clone()
        attn.sinks = nn.Parameter(local_sinks)

    orig_forward = attn.forward

    def forward(hidden_states, rotary_cos_sin):
        if sequence_parallel:
            hidden_states = _AllGatherSeq.apply(hidden_states, group, 1)
        else:
            hidden_states = _CopyToTP.apply(hidden_states, group)
        out = orig_forward(hidden_states, rotary_cos_sin)
        if sequence_parallel:
            return _ReduceScatterSeq.apply(out, group, 1)
        return _ReduceFromTP.apply(out, group)

    attn.forward = forward


def parallelize_tp_mlp(
    mlp: SwiGLU, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    _shard_linear(mlp.gate_proj, mesh, tp_dim, 0)
    _shard_linear(mlp.up_proj, mesh, tp_dim, 0)
    _shard_linear(mlp.down_proj, mesh, tp_dim, 1)

    orig_forward = mlp.forward

    def forward(x):
        if sequence_parallel:
            x = _AllGatherSeq.apply(x, group, 1)
        else:
            x = _CopyToTP.apply(x, group)
        out = orig_forward(x)
        if sequence_parallel:
            return _ReduceScatterSeq.apply(out, group, 1)
        return _ReduceFromTP.apply(out, group)

    mlp.forward = forward


def _slice_param_data(p: nn.Parameter, fn) -> nn.Parameter:
    """Replace a (possibly DTensor) parameter's data with fn(local)."""
    from torch.distributed.tensor import DTensor as _DT

    if isinstance(p.data, _DT):
        local = fn(p.data._local_tensor).contiguous()
        dt = _DT.from_local(
            local, p.data.device_mesh, p.data.placements, run_check=False
        )
        return nn.Parameter(dt, requires_grad=p.requires_grad)
    return nn.Parameter(fn(p.data).contiguous(), requires_grad=p.requires_grad)


def _shard_mlp_weights(mlp, mesh: DeviceMesh, tp_dim: int) -> None:
    """Colwise gate/up + rowwise down; NO boundary collectives (caller owns
    them so several partial producers can share one exit reduce)."""
    _shard_linear(mlp.gate_proj, mesh, tp_dim, 0)
    _shard_linear(mlp.up_proj, mesh, tp_dim, 0)
    _shard_linear(mlp.down_proj, mesh, tp_dim, 1)


def parallelize_tp_moe(
    moe, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    """TP over a MoELayer: experts' intermediate dim is sharded over tp.

    gate_up_proj (E, 2I, H) takes matching gate AND up slices (the packed
    [gate | up] layout shards as a permuted selection, so the weights stay
    PLAIN local tensors rather than DTensors — a Shard(1) placement would
    describe the wrong global layout for checkpoint gather); down_proj
    (E, H, I) takes the same intermediate slice. The router and (optional)
    shared expert stay replicated/sharded inside the layer and ALL partial
    outputs fold into ONE exit all-reduce (or SP reduce-scatter).
    Replicated params inside the region (router gate, shared-expert output
    gate) read through `_SumGradFromTP` so per-microbatch grads reduce
    exactly once. Apply BEFORE expert parallelism (EP wraps expert dim 0).

    Reference declares tp on every mesh domain but rejects tp > 1
    (d9d/core/dist_context/params.py:24-34); this is the real thing.
    """
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    rank = mesh.get_coordinate()[tp_dim]

    experts = moe.experts
    inter = experts.intermediate_size
    assert inter % tp_size == 0, "MoE intermediate size must divide tp"
    sh = inter // tp_size

    def gate_up_slice(w):  # (E, 2I, H) -> (E, 2*sh, H)
        gate = w[:, rank * sh : (rank + 1) * sh]
        up = w[:, inter + rank * sh : inter + (rank + 1) * sh]
        return torch.cat([gate, up], dim=1)

    def down_slice(w):  # (E, H, I) -> (E, H, sh)
        return w[:, :, rank * sh : (rank + 1) * sh]

    gl = experts.gate_up_proj
    gl._parameters["weight"] = _slice_param_data(gl._parameters["weight"], gate_up_slice)
    gl.out_features = 2 * sh
    dl = experts.down_proj
    dl._parameters["weight"] = _slice_param_data(dl._parameters["weight"], down_slice)
    dl.in_features = sh
    experts.intermediate_size = sh

    _install_tp_sumgrad(moe.router.gate, ("weight",), group)

    if moe.shared_expert is not None:
        se = moe.shared_expert
        assert se.gate_proj.out_features % tp_size == 0
        _shard_mlp_weights(se, mesh, tp_dim)
        if getattr(se, "use_gate", False):
            _install_tp_sumgrad(se.output_gate, ("weight",), group)

    orig_forward = moe.forward

    def forward(x):
        if sequence_parallel:
            x = _AllGatherSeq.apply(x, group, 1)
        else:
            x = _CopyToTP.apply(x, group)
        out = orig_forward(x)  # partial over tp (experts + shared expert)
        if sequence_parallel:
            return _ReduceScatterSeq.apply(out, group, 1)
        return _ReduceFromTP.apply(out, group)

    moe.forward = forward


def parallelize_tp_embeddings(
    emb, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    """Vocab-parallel SplitTokenEmbeddings: each segment's rows shard over
    tp (DTensor Shard(0)); out-of-shard tokens embed to zero through the
    module's existing segment masking, and the partial sums all-reduce at
    exit (SP: reduce-scatter along the sequence instead)."""
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    rank = mesh.get_coordinate()[tp_dim]

    for name in emb.order:
        seg = emb.embeddings[name]
        n = seg.num_embeddings
        assert n % tp_size == 0, f"vocab segment {name} must divide tp"
        sh = n // tp_size
        w = seg._parameters["weight"]
        local = w.data[rank * sh : (rank + 1) * sh].contiguous()
        placements: list[Placement] = [Replicate()] * mesh.ndim
        placements[tp_dim] = Shard(0)
        dt = DTensor.from_local(local, mesh, tuple(placements), run_check=False)
        seg._parameters["weight"] = nn.Parameter(dt, requires_grad=w.requires_grad)
        seg.num_embeddings = sh
        if not getattr(seg, "_d9d_to_local_params", None):
            seg.__class__ = _to_local_class(type(seg), ("weight",))
        # the masking window becomes this rank's global row range
        emb.offsets[name] = emb.offsets[name] + rank * sh

    orig_forward = emb.forward

    def forward(input_ids):
        out = orig_forward(input_ids)  # partial: off-shard tokens are zero
        if sequence_parallel:
            return _ReduceScatterSeq.apply(out, group, 1)
        return _ReduceFromTP.apply(out, group)

    emb.forward = forward


def parallelize_tp_lm_head(
    head, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    """Vocab-parallel SplitLanguageModellingHead over the existing
    vocab-parallel CCE op (ops/cce.py VocabParallelOptions): each segment's
    weight rows shard over tp; forward maps labels to local-concat indices
    (off-shard -> sentinel -7 so exactly one rank owns each target) and the
    fused loss merges lse/target across the group. Weight shards stay plain
    local tensors (ParameterDict entries; grads are complete per shard)."""
    from ..ops.cce import LM_IGNORE_INDEX, VocabParallelOptions, linear_cross_entropy

    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    rank = mesh.get_coordinate()[tp_dim]

    base_offsets = {}
    off = 0
    shard_sizes = {}
    for name in head.order:
        w = head.weights[name]
        n = w.shape[0]
        assert n % tp_size == 0, f"vocab segment {name} must divide tp"
        sh = n // tp_size
        base_offsets[name] = off
        shard_sizes[name] = sh
        off += n
        head.weights[name] = nn.Parameter(
            w.data[rank * sh : (rank + 1) * sh].contiguous(),
            requires_grad=w.requires_grad,
        )
    local_vocab = sum(shard_sizes.values())
    head._d9d_tp = (group, rank, base_offsets, shard_sizes, local_vocab)

    def tp_forward(hidden_states, labels):
        if sequence_parallel:
            # slice-backward gather: CCE's vocab-parallel backward already
            # all-reduces de over the group, so summing here would double it
            hidden_states = _AllGatherSeqSliceBwd.apply(hidden_states, group, 1)
        B, S, H = hidden_states.shape
        t = labels.reshape(-1)
        local_t = torch.full_like(t, -7)  # off-shard sentinel (not ignore)
        local_off = 0
        for name in head.order:
            start = base_offsets[name] + rank * shard_sizes[name]
            in_seg = (t >= start) & (t < start + shard_sizes[name])
            local_t = torch.where(in_seg, t - start + local_off, local_t)
            local_off += shard_sizes[name]
        local_t = torch.where(t == LM_IGNORE_INDEX, t, local_t)
        loss = linear_cross_entropy(
            hidden_states.reshape(-1, H),
            head.full_weight(),  # cat of local shards
            local_t,
            vocab_parallel=VocabParallelOptions(group, 0, local_off),
        )
        if sequence_parallel:
            # labels were full-sequence; loss follows the gathered sequence
            return (-loss).reshape(B, S)
        return (-loss).reshape(B, S)

    def tp_logits(hidden_states):
        local = (hidden_states @ head.full_weight().t()).contiguous()
        parts = [torch.empty_like(local) for _ in range(tp_size)]
        dist.all_gather(parts, local, group=group)
        # reassemble global vocab order from per-rank segment shards
        segs = []
        for r, part in enumerate(parts):
            off_l = 0
            seg_of_rank = {}
            for name in head.order:
                sh = shard_sizes[name]
                seg_of_rank[name] = part[..., off_l : off_l + sh]
                off_l += sh
            segs.append(seg_of_rank)
        out = []
        for name in head.order:
            out.extend(segs[r][name] for r in range(tp_size))
        return torch.cat(out, dim=-1)

    head.forward = tp_forward
    head.logits = tp_logits


def _wrap_tp_boundary(module: nn.Module, group, sequence_parallel: bool) -> None:
    """Entry copy-to-tp (SP: sequence all-gather), exit all-reduce (SP:
    reduce-scatter) around a block whose internals produce partial sums."""
    orig_forward = module.forward

    def forward(hidden_states, *args, **kwargs):
        if sequence_parallel:
            hidden_states = _AllGatherSeq.apply(hidden_states, group, 1)
        else:
            hidden_states = _CopyToTP.apply(hidden_states, group)
        out = orig_forward(hidden_states, *args, **kwargs)
        if sequence_parallel:
            return _ReduceScatterSeq.apply(out, group, 1)
        return _ReduceFromTP.apply(out, group)

    module.forward = forward


def parallelize_tp_mla(
    mla, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    """Head-parallel TP for MultiHeadLatentAttention: per-head projections
    (q up / kv up) shard colwise, o_proj rowwise; the shared latent path
    (kv_down, kv_norm, low-rank q down/norm) stays replicated inside the
    region with autograd-level tp-sum on its weights."""
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    assert mla.num_heads % tp_size == 0, "MLA heads must divide tp"

    q = mla.q_proj
    if isinstance(q, nn.Linear):
        _shard_linear(q, mesh, tp_dim, 0)
    else:  # LowRankProjection: shard the up matrix, replicate down + norm
        _shard_linear(q.up, mesh, tp_dim, 0)
        _install_tp_sumgrad(q.down, ("weight",), group)
        _install_tp_sumgrad(q.norm, ("weight",), group)
    _shard_linear(mla.kv_up, mesh, tp_dim, 0)
    _shard_linear(mla.o_proj, mesh, tp_dim, 1)
    _install_tp_sumgrad(mla.kv_down, ("weight",), group)
    _install_tp_sumgrad(mla.kv_norm, ("weight",), group)
    mla.num_heads //= tp_size
    _wrap_tp_boundary(mla, group, sequence_parallel)


def parallelize_tp_gdn(
    gdn, mesh: DeviceMesh, tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> None:
    """Head-parallel TP for GatedDeltaNet: q/k/v/beta/decay/out-gate
    projections and the causal-conv channels shard with the heads, o_proj
    rowwise; the per-head-dim output RMSNorm weight is shared across heads
    (replicated inside the region, tp-sum grads)."""
    from ..module.block.attention.linear import MambaDecayGate

    if isinstance(gdn.decay_gate, MambaDecayGate):
        raise NotImplementedError(
            "parallelize_tp_gdn does not shard the Mamba decay gate's A_log and dt_bias yet"
        )
    tp_dim = mesh.mesh_dim_names.index(tp_dim_name)
    tp_size = mesh.shape[tp_dim]
    if tp_size == 1:
        return
    group = mesh.get_group(tp_dim)
    rank = mesh.get_coordinate()[tp_dim]
    assert gdn.num_heads % tp_size == 0 and gdn.num_kv_heads % tp_size == 0

    def shard_conv(conv):
        w = conv._parameters["weight"]
        local = w.data.chunk(tp_size, dim=0)[rank].contiguous()
        placements: list[Placement] = [Replicate()] * mesh.ndim
        placements[tp_dim] = Shard(0)
        dt = DTensor.from_local(local, mesh, tuple(placements), run_check=False)
        conv._parameters["weight"] = nn.Parameter(dt, requires_grad=w.requires_grad)
        if not getattr(conv, "_d9d_to_local_params", None):
            conv.__class__ = _to_local_class(type(conv), ("weight",))

    for lin in (gdn.q_proj, gdn.k_proj, gdn.v_proj, gdn.beta_proj,
                gdn.decay_gate.proj, gdn.out_gate):
        _shard_linear(lin, mesh, tp_dim, 0)
    for conv in (gdn.q_conv, gdn.k_conv, gdn.v_conv):
        shard_conv(conv)
    _shard_linear(gdn.o_proj, mesh, tp_dim, 1)
    _install_tp_sumgrad(gdn.out_norm, ("weight",), group)
    gdn.num_heads //= tp_size
    gdn.num_kv_heads //= tp_size
    _wrap_tp_boundary(gdn, group, sequence_parallel)


def parallelize_tensor_parallel(
    module: nn.Module,
    mesh: DeviceMesh,
    tp_dim_name: str = "tp",
    sequence_parallel: bool = False,
) -> nn.Module:
    """Apply TP (optionally SP) to every GQA/MLA/GDN attention, SwiGLU FFN,
    MoE layer, split token embedding and split LM head in the module tree."""
    from ..module.block.attention import MultiHeadLatentAttention
    from ..module.block.attention.linear import GatedDeltaNet
    from ..module.block.embedding import SplitTokenEmbeddings
    from ..module.block.head import SplitLanguageModellingHead
    from ..module.block.moe import MoELayer

    if mesh.mesh_dim_names and "pp" in mesh.mesh_dim_names and mesh.ndim > 1:
        # stages hold different modules; placements must not span pp
        mesh = mesh[tuple(n for n in mesh.mesh_dim_names if n != "pp")]
    if sequence_parallel:
        tp_size = mesh.shape[mesh.mesh_dim_names.index(tp_dim_name)]
        for sub in module.modules():
            if hasattr(sub, "rotary"):
                # inter-block hidden states are sequence-sharded; the model
                # scales its position range back to the full sequence
                sub._d9d_sp_factor = tp_size
    for sub in module.modules():
        if isinstance(sub, GroupedQueryAttention):
            parallelize_tp_attention(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, MultiHeadLatentAttention):
            parallelize_tp_mla(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, GatedDeltaNet):
            parallelize_tp_gdn(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, MoELayer):
            parallelize_tp_moe(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, SwiGLU):
            parallelize_tp_mlp(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, SplitTokenEmbeddings):
            parallelize_tp_embeddings(sub, mesh, tp_dim_name, sequence_parallel)
        elif isinstance(sub, SplitLanguageModellingHead):
            parallelize_tp_lm_head(sub, mesh, tp_dim_name, sequence_parallel)
    return module
