"""Docstrings of oneflow.spmm / oneflow._C.fused_spmm_csr, in the add_docstr form of
python/oneflow/framework/docstr/math_ops.py (oneflow.mv, :1306).  A maintainer appends these
entries to math_ops.py; this file is not imported here (OneFlow is not installed)."""
import oneflow
from oneflow.framework.docstr.utils import add_docstr

add_docstr(
    oneflow.spmm,
    r"""
    spmm(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, static_csr=0) -> Tensor

    Multiplies the sparse matrix :math:`A` (:attr:`a_num_rows` :math:`\times` :attr:`a_num_cols`,
    CSR) by the dense matrix :attr:`b` (:attr:`a_num_cols` :math:`\times N`):
    :math:`out[r, :] = \sum_{j=rp[r]}^{rp[r+1]-1} values[j] \cdot b[col[j], :]`, summed in
    ascending :math:`j` (the order of gather -> multiply -> unsorted_segment_sum).

    Rows with more than ``T = clamp(65536 / N, 128, 512)`` nonzeros (rounded down to a power of
    two: 512 for N <= 128, 256 at N = 256, 128 from N = 512) are summed in chunks of ``T``
    nonzeros, the last chunk taking the remainder, and the chunk sums are then added in chunk
    order; the result is deterministic and identical on CPU and GPU.

    Column indices outside ``[0, a_num_cols)``: a column ``>= a_num_cols`` contributes
    ``value * 0`` in its place of the order (the gather's zero fill) on every device; a negative
    column raises on the CPU (the gather's CHECK) and contributes ``value * 0`` on the GPU (the
    CUDA gather's zero fill of any index outside the table).

    Args:
        a_csr_row_ptr (oneflow.Tensor): int32 or int64, shape ``[a_num_rows + 1]``
        a_csr_col_idx (oneflow.Tensor): same dtype as ``a_csr_row_ptr``, shape ``[nnz]``
        a_csr_values (oneflow.Tensor): float, double, float16 or bfloat16, shape ``[nnz]``
        a_num_rows (int): M
        a_num_cols (int): K
        b (oneflow.Tensor): dtype of ``a_csr_values``, shape ``[K, N]``
        static_csr (int, optional): 0 (default) plans the row work list on every call.  A non-zero
            value promises that the CSR tensors are not modified while calls carry that value;
            the GPU kernel then keeps the plan in its state and later calls skip the planning
            kernel.  Give a new CSR built in reused memory a new value.  No numeric effect.
    Returns:
        oneflow.Tensor: shape ``[M, N]``, dtype of ``b``

    Differentiable in ``a_csr_values`` (SDDMM) and ``b`` (:math:`A^T \cdot grad`).

    For example:

    .. code-block:: python

        >>> import oneflow as flow
        >>> row_ptr = flow.tensor([0, 2, 3], dtype=flow.int32)
        >>> col_idx = flow.tensor([0, 2, 1], dtype=flow.int32)
        >>> values = flow.tensor([1.0, 2.0, 3.0])
        >>> b = flow.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
        >>> flow.spmm(row_ptr, col_idx, values, 2, 3, b)
        tensor([[3., 2.],
                [0., 3.]], dtype=oneflow.float32)

    """,
)

add_docstr(
    oneflow._C.fused_spmm_csr,
    r"""
    fused_spmm_csr(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, bias=None, relu=False, static_csr=0) -> Tensor

    ``relu(spmm(...) + bias)`` in one kernel, with the bits of the three ops run separately
    (spmm, then bias_add over dim 1, then relu). ``bias`` has shape ``[N]``. ``static_csr`` as
    for ``oneflow.spmm``: a non-zero value keeps the plan of an unchanged CSR across calls.
    """,
)

add_docstr(
    oneflow._C.spmm_csr_reduce,
    r"""
    spmm_csr_reduce(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, reduce="sum") -> (Tensor, Tensor)

    ``oneflow.spmm`` with another aggregation over each row's products
    :math:`p_j = values[j] \cdot b[col[j], :]` (each rounded to the dtype of ``b``), as
    ``reduce=`` of a message-passing layer; ``oneflow.spmm(..., reduce=...)`` returns ``out`` alone.

    * ``"sum"``: ``oneflow.spmm``.
    * ``"mean"``: the sum divided by the row's number of nonzeros and rounded again (the bits of
      ``spmm`` followed by a broadcast divide); an empty row gives ``+0``.
    * ``"max"`` / ``"min"``: the elementwise extremum over the row's nonzeros.  Among equal
      candidates the lowest nonzero index wins (``+0`` and ``-0`` are equal); the first NaN wins
      and propagates, stored as the canonical quiet NaN.  An empty row gives ``+0``.  The result
      does not depend on any schedule and is identical on CPU and GPU.

    Returns:
        ``out`` of shape ``[M, N]`` and ``arg``: for ``"max"`` / ``"min"`` an ``[M, N]`` tensor of
        the index dtype holding the position in ``a_csr_col_idx`` / ``a_csr_values`` of the winning
        nonzero (``-1`` for an empty row); for ``"sum"`` / ``"mean"`` an empty ``[0, N]`` tensor.

    Differentiable in ``a_csr_values`` and ``b``; ``arg`` is not differentiable.  The gradient of
    ``"max"`` / ``"min"`` flows to the winning nonzero only and is deterministic: ``d(b)`` is
    accumulated in the order of ``spmm`` on :math:`A^T`, without atomics.

    For example:

    .. code-block:: python

        >>> import oneflow as flow
        >>> row_ptr = flow.tensor([0, 2, 3], dtype=flow.int32)
        >>> col_idx = flow.tensor([0, 2, 1], dtype=flow.int32)
        >>> values = flow.tensor([1.0, 2.0, 3.0])
        >>> b = flow.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
        >>> out, arg = flow._C.spmm_csr_reduce(row_ptr, col_idx, values, 2, 3, b, reduce="max")
        >>> out
        tensor([[2., 2.],
                [0., 3.]], dtype=oneflow.float32)
        >>> arg
        tensor([[1, 1],
                [2, 2]], dtype=oneflow.int32)

    """,
)

add_docstr(
    oneflow._C.gatv2_scores_csr_heads,
    r"""
    gatv2_scores_csr_heads(a_csr_row_ptr, a_csr_col_idx, x_row, x_col, att, num_heads, negative_slope=0.2) -> Tensor

    The attention scores of a GATv2 layer over a CSR pattern, in one launch:

    .. math::

        e_{j,h} = \sum_d att_{h,d} \cdot \mathrm{LeakyReLU}(x\_row_{row(j),h,d} + x\_col_{col_j,h,d})

    The activation sits between the gather and the dot product, so the score is neither a bilinear
    SDDMM nor a per-node scalar; the activated sum is rounded to the dtype and never written.

    Args:
        a_csr_row_ptr (Tensor): ``[M + 1]``, int32 or int64.
        a_csr_col_idx (Tensor): ``[nnz]``, the dtype of ``a_csr_row_ptr``.  A column outside
            ``[0, K)`` reads ``x_col`` as ``+0``.
        x_row (Tensor): ``[M, num_heads * D]``, the transformed destination features.
        x_col (Tensor): ``[K, num_heads * D]``, the transformed source features.
        att (Tensor): ``[num_heads * D]``, the attention vector of every head.
        num_heads (int): the number of heads; head ``h`` owns columns ``[h * D, (h + 1) * D)``.
        negative_slope (float): LeakyReLU's slope, finite and ``> 0``.

    Returns:
        ``out`` of shape ``[nnz, num_heads]``: exactly the bits of ``sddmm_csr_heads`` with the left
        row ``att`` and the right row the activated sum of the nonzero, identical on CPU and GPU.

    Differentiable in ``x_row``, ``x_col`` and ``att``.  The gradients are deterministic sums in the
    order of ``spmm_csr_heads`` (the one in ``x_col`` on :math:`A^T`), without atomics.  The
    softmax over each row (``edge_softmax_csr_heads``) and the aggregation (``spmm_csr_heads``) are
    separate ops.

    For example:

    .. code-block:: python

        >>> import oneflow as flow
        >>> row_ptr = flow.tensor([0, 2, 3], dtype=flow.int32)
        >>> col_idx = flow.tensor([0, 1, 1], dtype=flow.int32)
        >>> x_row = flow.tensor([[1.0, -1.0], [0.5, 0.5]])
        >>> x_col = flow.tensor([[1.0, 0.0], [-2.0, 0.0]])
        >>> att = flow.tensor([1.0, 1.0])
        >>> flow._C.gatv2_scores_csr_heads(row_ptr, col_idx, x_row, x_col, att, 1, 0.5)
        tensor([[ 1.5000],
                [-1.0000],
                [-0.2500]], dtype=oneflow.float32)

    """,
)

add_docstr(
    oneflow._C.spmm_csr_heads_fp8,
    r"""
    spmm_csr_heads_fp8(a_csr_row_ptr, a_csr_col_idx, a_csr_values, a_num_rows, a_num_cols, b, b_scale=None, b_format=1) -> Tensor

    The multi-head SpMM of ``spmm_csr_heads`` over a feature table stored in OCP FP8, one byte per
    element, with an optional scale per row of the table, in one launch:

    .. math::

        out_{r,hD+c} = \sum_{j \in row(r)} (values_{j,h} \cdot b\_scale_{col_j}) \cdot \mathrm{dequant}(b_{col_j,hD+c})

    The gathered rows of ``b`` are half the bytes of a bfloat16 table and a quarter of a float32
    one.  The sum is accumulated in float32.

    Args:
        a_csr_row_ptr (Tensor): ``[M + 1]``, int32 or int64.
        a_csr_col_idx (Tensor): ``[nnz]``, the dtype of ``a_csr_row_ptr``.  A column outside
            ``[0, K)`` reads a zero row of ``b`` and the scale ``+0``.
        a_csr_values (Tensor): ``[nnz, H]``, float32, float16 or bfloat16.
        a_num_rows (int), a_num_cols (int): ``M`` and ``K``.
        b (Tensor): ``[K, H * D]`` uint8, the FP8 codes; head ``h`` owns columns ``[h * D, (h + 1) * D)``.
        b_scale (Tensor, optional): ``[K]`` float32, the scale of every row of ``b``.
        b_format (int): 1 for ``e4m3fn`` (max 448), 2 for ``e5m2`` (max 57344).

    Returns:
        ``out`` of shape ``[M, H * D]`` and the dtype of ``a_csr_values``: exactly the bits of
        ``spmm_csr_heads`` on the values times ``b_scale[col]`` rounded to the dtype and on ``b``
        dequantised to the dtype (exact), identical on CPU and GPU.  Without ``b_scale`` the values
        are used as they are.

    Differentiable in ``a_csr_values`` only: the gradient is ``sddmm_csr_heads`` of the upstream
    gradient and the dequantised table, times ``b_scale[col]``.  That backward dequantises the whole
    table each time it runs.  ``b`` and ``b_scale`` have no gradient.

    For example:

    .. code-block:: python

        >>> import oneflow as flow
        >>> row_ptr = flow.tensor([0, 2, 3], dtype=flow.int32)
        >>> col_idx = flow.tensor([0, 1, 1], dtype=flow.int32)
        >>> values = flow.tensor([[1.0], [2.0], [4.0]])
        >>> b = flow.tensor([[0x38, 0x40], [0xB8, 0x30]], dtype=flow.uint8)  # e4m3fn: 1, 2; -1, 0.5
        >>> b_scale = flow.tensor([2.0, 0.5])
        >>> flow._C.spmm_csr_heads_fp8(row_ptr, col_idx, values, 2, 2, b, b_scale, 1)
        tensor([[ 1.0000,  4.5000],
                [-2.0000,  1.0000]], dtype=oneflow.float32)

    """,
)
