/*
 * spmm_functor.cpp — functional::SpmmCsr and its C-ABI entry (the Python binding calls this).
 *
 * Mirrors the functional layer of the reference: YAML signature
 *   "Tensor (Tensor a_csr_row_ptr, Tensor a_csr_col_idx, Tensor a_csr_values, Int64 a_num_rows,
 *            Int64 a_num_cols, Tensor b) => SpmmCsr"      (template functional_api.yaml:1062-1065)
 * and the functor pattern of oneflow/core/functional/impl/nn_functor.cpp:3861-3884 (argument
 * checks as RuntimeError, then OpInterpUtil::Dispatch).  "Dispatch" here is the eager-local
 * interpreter reduced to what one op needs (oneflow/core/framework/op_interpreter/
 * eager_local_op_interpreter.cpp:74-160): run the op's logical/dtype inference, choose the one
 * matching kernel (StatefulOpKernel::ChooseOpKernel, oneflow/user/kernels/stateful_opkernel.cpp:873-910),
 * init its cache (:912-935) and Compute on the device stream.  Output/tmp memory is owned by the
 * caller, as the VM owns it in the reference (oneflow/core/vm/op_call_instruction_policy.cpp:28-36).
 */
#include <mutex>

#include "oneflow/core/framework/framework.h"
#include "oneflow/core/functional/spmm_functor.h"
#include "ofx_internal.h"
#include "ofx_spmm.h"

namespace oneflow {
namespace {

using DescMap = std::map<std::pair<std::string, int32_t>, user_op::TensorDesc>;

Shape ShapeOf(const ofx_tensor_desc* d) {
  std::vector<int64_t> dims;
  for (int i = 0; i < d->ndim; ++i) dims.push_back(d->shape[i]);
  return Shape(dims);
}

int ToStatus(const Maybe<void>& m) {
  if (m.IsOk()) return OFX_OK;
  return ofx::fail(OFX_EINVAL, "%s: %s", m.kind().c_str(), m.message().c_str());
}

// A versioned descriptor (include/ofx_spmm.h): the tag, then struct_size at least the first
// tagged layout's.
Maybe<void> CheckDesc(const ofx_tensor_desc* d, const char* name) {
  const char* why = ofx::versioned_struct_problem(d, OFX_TENSOR_DESC_MIN_SIZE);
  CHECK_OR_RETURN(why == nullptr)
      << Error::RuntimeError() << name << ": ofx_tensor_desc " << why << " ("
      << OFX_TENSOR_DESC_MIN_SIZE << " bytes): initialise it with OFX_TENSOR_DESC_INIT";
  return Maybe<void>::Ok();
}

// Stride contract of the kernels: a 2-D tensor is rows of unit-stride elements at row_stride
// >= shape[1] (b may be a row-strided view; out too).  A column stride != 1 (e.g. out[:, ::2])
// cannot be expressed to the kernel, which takes only the row stride, and is refused.
Maybe<void> CheckUnitColumnStride(const ofx_tensor_desc* t, const char* name) {
  if (t->ndim == 2 && t->shape[0] > 0 && t->shape[1] > 1) {
    CHECK_OR_RETURN(t->stride[1] == 1 && t->stride[0] >= t->shape[1])
        << Error::RuntimeError() << "spmm_csr: " << name << " must have unit column stride and "
        << "row stride >= its columns, got strides (" << t->stride[0] << ", " << t->stride[1]
        << ")";
  }
  return Maybe<void>::Ok();
}

// Placement of a (possibly global) call: the hierarchy, out's NdSbp and b's NdSbp (out S(0) ->
// b B, out S(1) -> b S(1), out B -> b B), and this rank.  A local call is the 1-device placement.
struct Placement {
  Shape hierarchy{1};
  NdSbp out_sbp{"B"}, b_sbp{"B"};
  int64_t parallel_id = 0;
  int64_t parallel_num() const { return hierarchy.elem_cnt(); }
};

Maybe<void> MakePlacement(int hierarchy_ndim, const int64_t* hierarchy, const int32_t* out_split,
                          int64_t parallel_id, Placement* p) {
  CHECK_OR_RETURN(hierarchy_ndim >= 1 && hierarchy_ndim <= 4 && hierarchy && out_split)
      << Error::RuntimeError() << "spmm_csr: placement needs a 1-D..4-D hierarchy";
  std::vector<int64_t> dims;
  p->out_sbp.clear();
  p->b_sbp.clear();
  for (int i = 0; i < hierarchy_ndim; ++i) {
    CHECK_GE_OR_RETURN(hierarchy[i], 1) << Error::RuntimeError() << "bad hierarchy dim";
    CHECK_OR_RETURN(out_split[i] >= -1 && out_split[i] <= 1)
        << Error::RuntimeError() << "out can be split on axis 0 or 1 only";
    dims.push_back(hierarchy[i]);
    p->out_sbp.push_back(out_split[i] < 0 ? "B" : "S(" + std::to_string(out_split[i]) + ")");
    p->b_sbp.push_back(out_split[i] == 1 ? "S(1)" : "B");
  }
  p->hierarchy = Shape(dims);
  CHECK_OR_RETURN(parallel_id >= 0 && parallel_id < p->parallel_num())
      << Error::RuntimeError() << "spmm_csr: parallel_id " << parallel_id << " outside "
      << p->hierarchy.ToString();
  p->parallel_id = parallel_id;
  return Maybe<void>::Ok();
}

struct Arg {
  const char* name;
  const ofx_tensor_desc* d;
};

// What inference leaves for the dispatch: the op's attributes (the registered defaults, then the
// call's values), the physical inputs, and per output the NdSbp, the logical and the physical desc.
struct Inferred {
  user_op::AttrMap attrs;
  DescMap in;
  std::map<std::string, NdSbp> nd_sbp;
  std::map<std::string, user_op::TensorDesc> logical, physical;
};

// Inference of a registered user op on one rank of a placement (input "b" and every output follow
// the placement's NdSbp, the other inputs are broadcast): the op's logical rule on the logical b
// (K x b_logical_cols), then its physical rule on the physical inputs.
Maybe<void> InferUserOp(const std::string& op_name, const std::vector<Arg>& ins,
                        const user_op::AttrMap& call_attrs, const Placement& pl,
                        int64_t b_logical_cols, Inferred* r) {
  const user_op::OpRegistryResult* op = user_op::UserOpRegistryMgr::Get().GetOpRegistryResult(op_name);
  CHECK_OR_RETURN(op != nullptr) << Error::RuntimeError() << "op " << op_name << " is not registered";
  for (const auto& a : op->attrs) r->attrs[a.first] = a.second;
  for (const auto& a : call_attrs) r->attrs[a.first] = a.second;
  for (const Arg& a : ins)
    CHECK_OR_RETURN(a.d != nullptr) << Error::RuntimeError() << op_name << ": NULL input " << a.name;
  const int device = ins.front().d->device;
  for (const Arg& a : ins) {
    JUST(CheckDesc(a.d, a.name));
    CHECK_OR_RETURN(a.d->ndim >= 1 && a.d->ndim <= 2)
        << Error::RuntimeError() << op_name << ": " << a.name << " must be 1-D or 2-D";
    CHECK_EQ_OR_RETURN(a.d->device, device)
        << Error::RuntimeError() << op_name << ": expected all tensors on the same device";
    JUST(CheckUnitColumnStride(a.d, a.name));
    r->in[{a.name, 0}] = user_op::TensorDesc(ShapeOf(a.d), (DataType)a.d->dtype);
  }
  DescMap logical_in = r->in;
  auto b_it = logical_in.find({"b", 0});
  if (b_it != logical_in.end() && b_it->second.shape().NumAxes() == 2 && b_logical_cols >= 0) {
    Shape b_logical = b_it->second.shape();
    b_logical.Set(1, b_logical_cols);
    b_it->second = user_op::TensorDesc(b_logical, b_it->second.data_type());
  }
  user_op::InferContext lctx(logical_in, r->attrs);
  JUST(op->logical_infer(&lctx));
  JUST(op->dtype_infer(&lctx));
  r->nd_sbp["b"] = pl.b_sbp;
  for (const std::string& o : op->outputs) {
    r->nd_sbp[o] = pl.out_sbp;
    r->logical[o] = lctx.OutputTensorDesc(o, 0);
  }
  user_op::InferContext pctx(r->in, r->attrs);
  pctx.SetParallel(ParallelContext(pl.parallel_id, pl.parallel_num()), ParallelDesc(pl.hierarchy),
                   r->nd_sbp, r->logical);
  JUST(op->physical_infer(&pctx));
  JUST(op->dtype_infer(&pctx));
  for (const std::string& o : op->outputs) r->physical[o] = pctx.OutputTensorDesc(o, 0);
  return Maybe<void>::Ok();
}

// Kernel objects are shared and const, cached per registration (stateful_opkernel.cpp:887-908).
const user_op::OpKernel* GetKernel(const user_op::OpKernelRegistryResult* reg) {
  static std::mutex mu;
  static std::map<const void*, std::unique_ptr<user_op::OpKernel>> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto& slot = cache[reg];
  if (!slot) slot.reset(reg->create_fn());
  return slot.get();
}

// The eager op's kernel states: one per (kernel registration, device), as OneFlow's functor
// holds one op expression whose StatefulOpKernel keeps a state per device
// (stateful_opkernel.cpp:887-908).  Created on first use through CreateOpKernelState.
// Never destroyed: a state frees device memory, which must not happen from a static destructor
// after the HIP runtime has gone at process exit.
std::mutex g_eager_states_mu;
auto& g_eager_states =
    *new std::map<std::pair<const void*, int>, std::shared_ptr<user_op::OpKernelState>>();

user_op::OpKernelState* EagerKernelState(const user_op::OpKernelRegistryResult* reg,
                                         const user_op::OpKernel* kernel, int device,
                                         DeviceType dev) {
  std::lock_guard<std::mutex> lock(g_eager_states_mu);
  auto key = std::make_pair(static_cast<const void*>(reg), device);
  auto it = g_eager_states.find(key);
  if (it != g_eager_states.end()) return it->second.get();
  user_op::KernelInitContext ictx(ParallelContext(0, 1), ParallelDesc(Shape({1})), dev);
  auto st = kernel->CreateOpKernelState(&ictx);
  user_op::OpKernelState* raw = st.get();
  g_eager_states[key] = std::move(st);
  return raw;
}

// Eager dispatch of a registered user op on one rank of a placement (a local call is the 1-device
// placement): inference -> kernel choice (HOB on every arg's dtype) -> the tmp size (tmp_size_out
// != NULL) or output check, the kernel's cache init and Compute on the stream.  `state`: the
// compiled job's own kernel state (NULL: the eager op's, per registration and device, and only
// for a static CSR).
Maybe<void> RunUserOp(const std::string& op_name, const std::vector<Arg>& ins,
                      const std::vector<Arg>& outs, const user_op::AttrMap& call_attrs, void* stream,
                      void* tmp, size_t tmp_bytes, size_t* tmp_size_out,
                      const Placement& pl = Placement(), int64_t b_logical_cols = -1,
                      int num_threads = 0,
                      std::shared_ptr<user_op::OpKernelState>* state = nullptr) {
  Inferred inf;
  JUST(InferUserOp(op_name, ins, call_attrs, pl, b_logical_cols, &inf));
  const int device = ins.front().d->device;
  user_op::KernelRegContext rc;
  rc.device_type_ = device < 0 ? DeviceType::kCPU : DeviceType::kHIP;
  for (const Arg& a : ins) rc.dtypes[{a.name, 0}] = (DataType)a.d->dtype;
  for (const auto& o : inf.physical) rc.dtypes[{o.first, 0}] = o.second.data_type();
  const user_op::OpKernelRegistryResult* reg = nullptr;
  JUST(user_op::UserOpRegistryMgr::Get().GetOpKernelRegistryResult(op_name, rc, &reg));
  if (tmp_size_out) {
    user_op::InferSizeContext sc;
    sc.descs = inf.in;
    sc.attrs = inf.attrs;
    sc.logical = inf.logical;
    *tmp_size_out = reg->infer_tmp_size ? reg->infer_tmp_size(&sc) : 0;
    return Maybe<void>::Ok();
  }
  std::vector<std::unique_ptr<user_op::Tensor>> hold;
  std::map<std::pair<std::string, int32_t>, user_op::Tensor*> tensors;
  auto add = [&](const Arg& a) {
    hold.emplace_back(new user_op::Tensor(ShapeOf(a.d), (DataType)a.d->dtype, a.d->data,
                                          a.d->ndim == 2 ? a.d->stride[0] : -1));
    tensors[{a.name, 0}] = hold.back().get();
  };
  for (const Arg& a : ins) add(a);
  bool all_outputs_empty = true;
  for (const Arg& o : outs) {
    CHECK_OR_RETURN(o.d != nullptr) << Error::RuntimeError() << op_name << ": NULL output " << o.name;
    JUST(CheckDesc(o.d, o.name));
    const user_op::TensorDesc& want = inf.physical.at(o.name);
    CHECK_OR_RETURN(ShapeOf(o.d) == want.shape() && (DataType)o.d->dtype == want.data_type() &&
                    o.d->device == device)
        << Error::RuntimeError() << op_name << ": output " << o.name << " must be "
        << want.shape().ToString() << " of dtype " << DataType_Name(want.data_type());
    JUST(CheckUnitColumnStride(o.d, o.name));
    add(o);
    all_outputs_empty = all_outputs_empty && want.shape().elem_cnt() == 0;
  }
  user_op::Tensor t_tmp(Shape({(int64_t)tmp_bytes}), kChar, tmp);
  if (tmp) tensors[{"tmp_buffer", 0}] = &t_tmp;
  ep::CpuStream cpu_stream(num_threads);
  ep::HipStream hip_stream(stream, device);
  ep::Stream* s = device < 0 ? static_cast<ep::Stream*>(&cpu_stream) : static_cast<ep::Stream*>(&hip_stream);
  user_op::KernelComputeContext ctx(s, tensors, inf.attrs, rc.device_type());
  const user_op::OpKernel* kernel = GetKernel(reg);
  const ParallelContext pc(pl.parallel_id, pl.parallel_num());
  auto sc = inf.attrs.find("static_csr");
  user_op::OpKernelState* kstate = nullptr;
  if (state != nullptr) {
    if (!*state) {
      // a compiled op's launches are ordered on its one (named) stream
      user_op::KernelInitContext ictx(pc, ParallelDesc(pl.hierarchy), rc.device_type(),
                                      "compiled_job");
      *state = kernel->CreateOpKernelState(&ictx);
    }
    kstate = state->get();
  } else if (sc != inf.attrs.end() && static_cast<int64_t>(sc->second) != 0) {
    // a static CSR's plan lives in the eager op's kernel state (per registration and device)
    kstate = EagerKernelState(reg, kernel, device, rc.device_type());
  }
  user_op::KernelCacheContext cache_ctx(pc, ParallelDesc(pl.hierarchy), inf.nd_sbp, inf.logical,
                                        rc.device_type());
  try {
    std::shared_ptr<user_op::OpKernelCache> cache = kernel->InitOpKernelCache(&cache_ctx);
    if (all_outputs_empty && !kernel->AlwaysComputeWhenAllOutputsEmpty()) return Maybe<void>::Ok();
    kernel->Compute(&ctx, kstate, cache.get());
  } catch (const KernelCheckError& e) {
    return Maybe<void>("KernelCheckError", e.msg);
  }
  return Maybe<void>::Ok();
}

// The call's ofx_spmm_attrs (NULL: the defaults), checked as a versioned struct: its static_csr.
int ReadStaticCsr(const ofx_spmm_attrs* attrs, const char* op_name, int64_t* static_csr) {
  *static_csr = 0;
  if (attrs == nullptr) return OFX_OK;
  const uint32_t min_size = OFX_SPMM_ATTRS_MIN_SIZE;
  const char* why = ofx::versioned_struct_problem(attrs, min_size);
  OFX_REQUIRE(why == nullptr, OFX_EINVAL,
              "%s: ofx_spmm_attrs %s (%u bytes): initialise it with OFX_SPMM_ATTRS_INIT", op_name,
              why ? why : "", min_size);
  *static_csr = attrs->static_csr;
  return OFX_OK;
}

// functional::SpmmCsr on a local or global tensor set.
int SpmmCsr(void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
            const ofx_tensor_desc* values, int64_t m, int64_t k, const ofx_tensor_desc* b,
            int64_t b_logical_cols, ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
            const Placement& pl, int num_threads, size_t* tmp_size_out, int64_t static_csr = 0,
            std::shared_ptr<user_op::OpKernelState>* state = nullptr) {
  // an earlier launch's loud failure comes back here as OFX_EPLAN, before this call launches
  // (the functional call is a library entry like ofx_spmm_csr)
  if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr");
  return ToStatus(RunUserOp("spmm_csr",
                            {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                             {"a_csr_values", values}, {"b", b}},
                            {{"out", out}},
                            {{"a_num_rows", m}, {"a_num_cols", k}, {"static_csr", static_csr}},
                            stream, tmp, tmp_bytes, tmp_size_out, pl, b_logical_cols, num_threads,
                            state));
}

}  // namespace

int SpmmCsrGlobalWithState(void* stream, const ofx_tensor_desc* row_ptr,
                           const ofx_tensor_desc* col_idx, const ofx_tensor_desc* values,
                           int64_t m, int64_t k, const ofx_tensor_desc* b, int64_t b_logical_cols,
                           ofx_tensor_desc* out, void* tmp, size_t tmp_bytes, int hierarchy_ndim,
                           const int64_t* hierarchy, const int32_t* out_split_axes,
                           int64_t parallel_id, int64_t static_csr,
                           std::shared_ptr<user_op::OpKernelState>* state) {
  Placement pl;
  int rc = ToStatus(MakePlacement(hierarchy_ndim, hierarchy, out_split_axes, parallel_id, &pl));
  if (rc) return rc;
  return SpmmCsr(stream, row_ptr, col_idx, values, m, k, b, b_logical_cols, out, tmp, tmp_bytes,
                 pl, 0, nullptr, static_csr, state);
}

}  // namespace oneflow

using namespace oneflow;

extern "C" int ofx_functional_spmm_csr_infer(const ofx_tensor_desc* row_ptr,
                                             const ofx_tensor_desc* col_idx,
                                             const ofx_tensor_desc* values, int64_t a_num_rows,
                                             int64_t a_num_cols, const ofx_tensor_desc* b,
                                             ofx_tensor_desc* out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    Inferred inf;
    int rc = ToStatus(InferUserOp("spmm_csr",
                                  {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                                   {"a_csr_values", values}, {"b", b}},
                                  {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols}},
                                  Placement(), -1, &inf));
    if (rc) return rc;
    rc = ToStatus(CheckDesc(out, "out"));
    if (rc) return rc;
    const user_op::TensorDesc& od = inf.physical.at("out");
    if (out) {
      out->dtype = od.data_type();
      out->ndim = (int32_t)od.shape().NumAxes();
      for (int i = 0; i < out->ndim; ++i) out->shape[i] = od.shape().At(i);
      out->device = b->device;
    }
    return OFX_OK;
  });
}

extern "C" int ofx_functional_spmm_csr_tmp_size(const ofx_tensor_desc* row_ptr,
                                                const ofx_tensor_desc* col_idx,
                                                const ofx_tensor_desc* values, int64_t a_num_rows,
                                                int64_t a_num_cols, const ofx_tensor_desc* b,
                                                size_t* bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(bytes, OFX_EINVAL, "spmm_csr_tmp_size: bytes is NULL");
    return SpmmCsr(nullptr, row_ptr, col_idx, values, a_num_rows, a_num_cols, b, -1, nullptr,
                   nullptr, 0, Placement(), 0, bytes);
  });
}

extern "C" int ofx_functional_spmm_csr_global(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, int64_t a_num_rows, int64_t a_num_cols,
    const ofx_tensor_desc* b, int64_t b_logical_cols, ofx_tensor_desc* out, void* tmp,
    size_t tmp_bytes, int hierarchy_ndim, const int64_t* hierarchy, const int32_t* out_split_axes,
    int64_t parallel_id, int num_threads, size_t* tmp_size_out) {
  return ofx_functional_spmm_csr_global_attrs(stream, row_ptr, col_idx, values, a_num_rows,
                                              a_num_cols, b, b_logical_cols, out, tmp, tmp_bytes,
                                              hierarchy_ndim, hierarchy, out_split_axes,
                                              parallel_id, num_threads, tmp_size_out, nullptr);
}

extern "C" int ofx_functional_spmm_csr_global_attrs(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, int64_t a_num_rows, int64_t a_num_cols,
    const ofx_tensor_desc* b, int64_t b_logical_cols, ofx_tensor_desc* out, void* tmp,
    size_t tmp_bytes, int hierarchy_ndim, const int64_t* hierarchy, const int32_t* out_split_axes,
    int64_t parallel_id, int num_threads, size_t* tmp_size_out, const ofx_spmm_attrs* attrs) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int64_t static_csr;
    if (int rc = ReadStaticCsr(attrs, "spmm_csr", &static_csr)) return rc;
    Placement pl;
    if (int rc = ToStatus(MakePlacement(hierarchy_ndim, hierarchy, out_split_axes, parallel_id, &pl)))
      return rc;
    return SpmmCsr(stream, row_ptr, col_idx, values, a_num_rows, a_num_cols, b, b_logical_cols,
                   out, tmp, tmp_bytes, pl, num_threads, tmp_size_out, static_csr);
  });
}

extern "C" int ofx_spmm_static_plans(int64_t* entries, int64_t* plans, int64_t* hits,
                                     int release) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int64_t e = 0, p = 0, h = 0;
    std::lock_guard<std::mutex> lock(g_eager_states_mu);
    for (auto& kv : g_eager_states)
      if (kv.second) SpmmCsrPlanStateStats(kv.second.get(), &e, &p, &h, release != 0);
    if (entries) *entries = e;
    if (plans) *plans = p;
    if (hits) *hits = h;
    return OFX_OK;
  });
}

extern "C" int ofx_functional_spmm_csr_ex(void* stream, const ofx_tensor_desc* row_ptr,
                                          const ofx_tensor_desc* col_idx,
                                          const ofx_tensor_desc* values, int64_t a_num_rows,
                                          int64_t a_num_cols, const ofx_tensor_desc* b,
                                          ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
                                          int64_t parallel_id, int64_t parallel_num,
                                          int out_split_axis, int num_threads) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(out_split_axis != 1 || parallel_num == 1, OFX_EINVAL,
                "spmm_csr_ex: a column split needs the logical width: use "
                "ofx_functional_spmm_csr_global");
    const int64_t h = parallel_num;
    const int32_t ax = out_split_axis;
    return ofx_functional_spmm_csr_global(stream, row_ptr, col_idx, values, a_num_rows, a_num_cols,
                                          b, -1, out, tmp, tmp_bytes, 1, &h, &ax, parallel_id,
                                          num_threads, nullptr);
  });
}

extern "C" int ofx_functional_spmm_csr(void* stream, const ofx_tensor_desc* row_ptr,
                                       const ofx_tensor_desc* col_idx,
                                       const ofx_tensor_desc* values, int64_t a_num_rows,
                                       int64_t a_num_cols, const ofx_tensor_desc* b,
                                       ofx_tensor_desc* out, void* tmp, size_t tmp_bytes) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return SpmmCsr(stream, row_ptr, col_idx, values, a_num_rows, a_num_cols, b, -1, out, tmp,
                   tmp_bytes, Placement(), 0, nullptr);
  });
}

// SBP signatures of a registered op, for the tests: "arg:sbp,arg:sbp;...|no_grad:..." into buf.
// `optional_inputs`: comma-separated optional inputs the op instance has (e.g. "bias").
extern "C" int ofx_op_sbp_signatures(const char* op_name, const char* optional_inputs, char* buf,
                                     size_t len) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(op_name && buf && len > 0, OFX_EINVAL, "op_sbp_signatures: NULL argument");
    const user_op::OpRegistryResult* op = user_op::UserOpRegistryMgr::Get().GetOpRegistryResult(op_name);
    OFX_REQUIRE(op, OFX_EINVAL, "op %s is not registered", op_name);
    std::vector<std::string> present;
    if (optional_inputs) {
      std::string all(optional_inputs), cur;
      for (char ch : all + ",") {
        if (ch == ',') {
          if (!cur.empty()) present.push_back(cur);
          cur.clear();
        } else {
          cur += ch;
        }
      }
    }
    user_op::SbpContext ctx{user_op::UserOpConfView(present)};
    int rc = ToStatus(op->get_sbp(&ctx));
    if (rc) return rc;
    std::string s;
    for (const auto& sig : ctx.signatures()) {
      if (!s.empty()) s += ";";
      for (size_t i = 0; i < sig.size(); ++i) s += (i ? "," : "") + sig[i].first + ":" + sig[i].second;
    }
    // input-arg modifiers: which inputs have requires_grad disabled
    std::map<std::string, user_op::InputArgModifier> mods;
    user_op::GetInputArgModifier get = [&](const std::string& n, int32_t) { return &mods[n]; };
    if (op->input_modify) {
      rc = ToStatus(op->input_modify(get, user_op::UserOpConfWrapper()));
      if (rc) return rc;
    }
    s += "|no_grad:";
    bool first = true;
    for (const auto& kv : mods)
      if (!kv.second.requires_grad) {
        s += (first ? "" : ",") + kv.first;
        first = false;
      }
    snprintf(buf, len, "%s", s.c_str());
    return OFX_OK;
  });
}

extern "C" int ofx_op_spmm_csr_sbp_signatures(char* buf, size_t len) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return ofx_op_sbp_signatures("spmm_csr", nullptr, buf, len);
  });
}

// ---- gradient functors: functional::SddmmCsr / functional::CsrTranspose ----------------------
// The grad function of spmm_csr calls these; the Python autograd binding
// (oneflow_spmm/autograd.py) goes through the same entries.  Through RunUserOp, as every op.
extern "C" int ofx_functional_sddmm_csr(void* stream, const ofx_tensor_desc* row_ptr,
                                        const ofx_tensor_desc* col_idx, const ofx_tensor_desc* a,
                                        const ofx_tensor_desc* b, int64_t a_num_rows,
                                        int64_t a_num_cols, ofx_tensor_desc* out, void* tmp,
                                        size_t tmp_bytes, size_t* tmp_size_out) {
  return ofx_functional_sddmm_csr_attrs(stream, row_ptr, col_idx, a, b, a_num_rows, a_num_cols,
                                        out, tmp, tmp_bytes, tmp_size_out, nullptr);
}

// The same with the op's other attributes (static_csr: the SDDMM's plan of an unchanged CSR is
// kept in the eager op's kernel state -- the values-gradient of a static graph).
extern "C" int ofx_functional_sddmm_csr_attrs(void* stream, const ofx_tensor_desc* row_ptr,
                                              const ofx_tensor_desc* col_idx,
                                              const ofx_tensor_desc* a, const ofx_tensor_desc* b,
                                              int64_t a_num_rows, int64_t a_num_cols,
                                              ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
                                              size_t* tmp_size_out, const ofx_spmm_attrs* attrs) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int64_t static_csr;
    if (int rc = ReadStaticCsr(attrs, "sddmm_csr", &static_csr)) return rc;
    return ToStatus(RunUserOp("sddmm_csr",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"a", a}, {"b", b}},
                              {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols},
                               {"static_csr", static_csr}},
                              stream, tmp, tmp_bytes, tmp_size_out));
  });
}

extern "C" int ofx_functional_csr_transpose(void* stream, const ofx_tensor_desc* row_ptr,
                                            const ofx_tensor_desc* col_idx, int64_t a_num_rows,
                                            int64_t a_num_cols, ofx_tensor_desc* out_row_ptr,
                                            ofx_tensor_desc* out_col_idx, ofx_tensor_desc* out_perm,
                                            void* tmp, size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    return ToStatus(RunUserOp("csr_transpose", {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}},
                              {{"out_row_ptr", out_row_ptr}, {"out_col_idx", out_col_idx}, {"out_perm", out_perm}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols}}, stream, tmp,
                              tmp_bytes, tmp_size_out));
  });
}

// functional::SpmmCsrGathered: the d(b) gradient of spmm_csr with learnable values, A^T's
// structure with A's values read through A^T's perm.
extern "C" int ofx_functional_spmm_csr_gathered(void* stream, const ofx_tensor_desc* row_ptr,
                                                const ofx_tensor_desc* col_idx,
                                                const ofx_tensor_desc* values,
                                                const ofx_tensor_desc* values_perm,
                                                const ofx_tensor_desc* b, int64_t a_num_rows,
                                                int64_t a_num_cols, ofx_tensor_desc* out,
                                                void* tmp, size_t tmp_bytes,
                                                size_t* tmp_size_out) {
  return ofx_functional_spmm_csr_gathered_attrs(stream, row_ptr, col_idx, values, values_perm, b,
                                                a_num_rows, a_num_cols, out, tmp, tmp_bytes,
                                                tmp_size_out, nullptr);
}

// The same with the op's other attributes (static_csr: autograd's cached A^T keeps its plan).
extern "C" int ofx_functional_spmm_csr_gathered_attrs(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, const ofx_tensor_desc* values_perm, const ofx_tensor_desc* b,
    int64_t a_num_rows, int64_t a_num_cols, ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
    size_t* tmp_size_out, const ofx_spmm_attrs* attrs) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int64_t static_csr;
    if (int rc = ReadStaticCsr(attrs, "spmm_csr_gathered", &static_csr)) return rc;
    return ToStatus(RunUserOp("spmm_csr_gathered",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                               {"a_csr_values", values}, {"values_perm", values_perm}, {"b", b}},
                              {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols},
                               {"static_csr", static_csr}},
                              stream, tmp, tmp_bytes, tmp_size_out));
  });
}

// functional::FusedSpmmCsr: relu?(A @ b + bias?) through op
// "fused_spmm_csr"; `bias` may be NULL (the optional input is then absent).
extern "C" int ofx_functional_fused_spmm_csr(void* stream, const ofx_tensor_desc* row_ptr,
                                             const ofx_tensor_desc* col_idx,
                                             const ofx_tensor_desc* values,
                                             const ofx_tensor_desc* b, const ofx_tensor_desc* bias,
                                             int64_t a_num_rows, int64_t a_num_cols, int relu,
                                             ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
                                             size_t* tmp_size_out) {
  return ofx_functional_fused_spmm_csr_attrs(stream, row_ptr, col_idx, values, b, bias,
                                             a_num_rows, a_num_cols, relu, out, tmp, tmp_bytes,
                                             tmp_size_out, nullptr);
}

// The same with the op's other attributes (static_csr: the plan kept in the eager op's kernel
// state, as for spmm_csr).
extern "C" int ofx_functional_fused_spmm_csr_attrs(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, const ofx_tensor_desc* b, const ofx_tensor_desc* bias,
    int64_t a_num_rows, int64_t a_num_cols, int relu, ofx_tensor_desc* out, void* tmp,
    size_t tmp_bytes, size_t* tmp_size_out, const ofx_spmm_attrs* attrs) {
  return ::ofx::guarded(__func__, [&]() -> int {
    int64_t static_csr;
    if (int rc = ReadStaticCsr(attrs, "fused_spmm_csr", &static_csr)) return rc;
    // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("fused_spmm_csr");
    std::vector<Arg> ins = {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                            {"a_csr_values", values}, {"b", b}};
    if (bias != nullptr) ins.push_back({"bias", bias});
    return ToStatus(RunUserOp("fused_spmm_csr", ins, {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols},
                               {"relu", relu ? 1 : 0}, {"static_csr", static_csr}},
                              stream, tmp, tmp_bytes, tmp_size_out));
  });
}

// ---- functional::SpmmCsrReduce and its gradient functors ----------------------------------------
// Ops "spmm_csr_reduce" (sum / mean / max / min with the arg output), "spmm_csr_reduce_grad_b" and
// "spmm_csr_reduce_grad_values" through the same op-registry dispatch.
extern "C" int ofx_functional_spmm_csr_reduce(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, int64_t a_num_rows, int64_t a_num_cols, const ofx_tensor_desc* b,
    int reduce, ofx_tensor_desc* out, ofx_tensor_desc* arg, void* tmp, size_t tmp_bytes,
    int64_t parallel_id, int64_t parallel_num, int out_split_axis, int64_t b_logical_cols,
    int num_threads, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(reduce >= OFX_REDUCE_SUM && reduce <= OFX_REDUCE_MIN, OFX_EINVAL,
                "spmm_csr_reduce: unknown reduce code %d (OFX_REDUCE_SUM/MEAN/MAX/MIN)", reduce);
    // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr_reduce");
    Placement pl;
    const int64_t hierarchy = parallel_num;
    const int32_t axis = out_split_axis;
    int rc = ToStatus(MakePlacement(1, &hierarchy, &axis, parallel_id, &pl));
    if (rc) return rc;
    std::vector<Arg> outs;
    if (tmp_size_out == nullptr) outs = {{"out", out}, {"arg", arg}};
    return ToStatus(RunUserOp("spmm_csr_reduce",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                               {"a_csr_values", values}, {"b", b}},
                              outs,
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols},
                               {"reduce", reduce}},
                              stream, tmp, tmp_bytes, tmp_size_out, pl, b_logical_cols,
                              num_threads));
  });
}

extern "C" int ofx_functional_spmm_csr_reduce_grad_b(
    void* stream, const ofx_tensor_desc* at_row_ptr, const ofx_tensor_desc* at_col_idx,
    const ofx_tensor_desc* at_perm, const ofx_tensor_desc* values, const ofx_tensor_desc* arg,
    const ofx_tensor_desc* dy, int64_t a_num_rows, int64_t a_num_cols, ofx_tensor_desc* out,
    void* tmp, size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(arg != nullptr, OFX_EINVAL,
                "spmm_csr_reduce_grad_b: arg is NULL (the gradient of max / min needs it)");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr_reduce_grad_b");
    return ToStatus(RunUserOp("spmm_csr_reduce_grad_b",
                              {{"at_row_ptr", at_row_ptr}, {"at_col_idx", at_col_idx},
                               {"at_perm", at_perm}, {"a_csr_values", values}, {"arg", arg},
                               {"dy", dy}},
                              {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols}}, stream,
                              tmp, tmp_bytes, tmp_size_out));
  });
}

extern "C" int ofx_functional_spmm_csr_reduce_grad_values(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* arg, const ofx_tensor_desc* dy, const ofx_tensor_desc* b,
    int64_t a_num_rows, int64_t a_num_cols, ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
    size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(arg != nullptr, OFX_EINVAL,
                "spmm_csr_reduce_grad_values: arg is NULL (the gradient of max / min needs it)");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr_reduce_grad_values");
    return ToStatus(RunUserOp("spmm_csr_reduce_grad_values",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                               {"arg", arg}, {"dy", dy}, {"b", b}},
                              {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols}}, stream,
                              tmp, tmp_bytes, tmp_size_out));
  });
}

// ---- functional::EdgeSoftmaxCsr and its gradient functor ----------------------------------------
// Ops "edge_softmax_csr" and "edge_softmax_csr_grad" (oneflow/user/ops/edge_softmax_op.cpp)
// through the same op-registry dispatch.
namespace oneflow {

int EdgeSoftmaxCsr(void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
                   const ofx_tensor_desc* in, const ofx_tensor_desc* grad, ofx_tensor_desc* out,
                   void* tmp, size_t tmp_bytes, size_t* tmp_size_out, int num_threads) {
  // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
  if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("edge_softmax_csr");
  if (grad == nullptr)
    return ToStatus(RunUserOp("edge_softmax_csr",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"e", in}},
                              {{"out", out}}, {}, stream, tmp, tmp_bytes, tmp_size_out, Placement(), -1,
                              num_threads));
  return ToStatus(RunUserOp("edge_softmax_csr_grad",
                            {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"y", in},
                             {"dy", grad}},
                            {{"dx", out}}, {}, stream, tmp, tmp_bytes, tmp_size_out, Placement(), -1,
                            num_threads));
}

}  // namespace oneflow

extern "C" int ofx_functional_edge_softmax_csr(void* stream, const ofx_tensor_desc* row_ptr,
                                               const ofx_tensor_desc* col_idx,
                                               const ofx_tensor_desc* e, ofx_tensor_desc* out,
                                               void* tmp, size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(e != nullptr, OFX_EINVAL, "edge_softmax_csr: NULL input e");
    return EdgeSoftmaxCsr(stream, row_ptr, col_idx, e, nullptr, out, tmp, tmp_bytes, tmp_size_out,
                          0);
  });
}

extern "C" int ofx_functional_edge_softmax_csr_grad(void* stream, const ofx_tensor_desc* row_ptr,
                                                    const ofx_tensor_desc* col_idx,
                                                    const ofx_tensor_desc* y,
                                                    const ofx_tensor_desc* dy, ofx_tensor_desc* dx,
                                                    void* tmp, size_t tmp_bytes,
                                                    size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(y != nullptr && dy != nullptr, OFX_EINVAL,
                "edge_softmax_csr_grad: NULL input y or dy");
    return EdgeSoftmaxCsr(stream, row_ptr, col_idx, y, dy, dx, tmp, tmp_bytes, tmp_size_out, 0);
  });
}

// ---- functional::SpmmCsrHeads / SddmmCsrHeads ---------------------------------------------------
// Ops "spmm_csr_heads" and "sddmm_csr_heads" (oneflow/user/ops/spmm_heads_op.cpp) through the same
// op-registry dispatch.
extern "C" int ofx_functional_spmm_csr_heads(void* stream, const ofx_tensor_desc* row_ptr,
                                             const ofx_tensor_desc* col_idx,
                                             const ofx_tensor_desc* values,
                                             const ofx_tensor_desc* b, int64_t a_num_rows,
                                             int64_t a_num_cols, ofx_tensor_desc* out, void* tmp,
                                             size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(values != nullptr && b != nullptr, OFX_EINVAL,
                "spmm_csr_heads: NULL input a_csr_values or b");
    // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr_heads");
    return ToStatus(RunUserOp("spmm_csr_heads",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                               {"a_csr_values", values}, {"b", b}},
                              {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols}}, stream,
                              tmp, tmp_bytes, tmp_size_out));
  });
}

extern "C" int ofx_functional_sddmm_csr_heads(void* stream, const ofx_tensor_desc* row_ptr,
                                              const ofx_tensor_desc* col_idx,
                                              const ofx_tensor_desc* a, const ofx_tensor_desc* b,
                                              int64_t num_heads, ofx_tensor_desc* out, void* tmp,
                                              size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(a != nullptr && b != nullptr, OFX_EINVAL, "sddmm_csr_heads: NULL input a or b");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("sddmm_csr_heads");
    return ToStatus(RunUserOp("sddmm_csr_heads",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"a", a},
                               {"b", b}},
                              {{"out", out}}, {{"num_heads", num_heads}}, stream, tmp, tmp_bytes,
                              tmp_size_out));
  });
}

// ---- functional::EdgeSoftmaxCsrHeads and its gradient functor -----------------------------------
// Ops "edge_softmax_csr_heads" and "edge_softmax_csr_heads_grad"
// (oneflow/user/ops/edge_softmax_heads_op.cpp) through the same op-registry dispatch
// (INTEGRATION.md §11).
namespace oneflow {

int EdgeSoftmaxCsrHeads(void* stream, const ofx_tensor_desc* row_ptr,
                        const ofx_tensor_desc* col_idx, const ofx_tensor_desc* in,
                        const ofx_tensor_desc* grad, ofx_tensor_desc* out, void* tmp,
                        size_t tmp_bytes, size_t* tmp_size_out, int num_threads) {
  // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
  if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("edge_softmax_csr_heads");
  if (grad == nullptr)
    return ToStatus(RunUserOp("edge_softmax_csr_heads",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"e", in}},
                              {{"out", out}}, {}, stream, tmp, tmp_bytes, tmp_size_out, Placement(), -1,
                              num_threads));
  return ToStatus(RunUserOp("edge_softmax_csr_heads_grad",
                            {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"y", in},
                             {"dy", grad}},
                            {{"dx", out}}, {}, stream, tmp, tmp_bytes, tmp_size_out, Placement(), -1,
                            num_threads));
}

}  // namespace oneflow

extern "C" int ofx_functional_edge_softmax_csr_heads(void* stream, const ofx_tensor_desc* row_ptr,
                                                     const ofx_tensor_desc* col_idx,
                                                     const ofx_tensor_desc* e, ofx_tensor_desc* out,
                                                     void* tmp, size_t tmp_bytes,
                                                     size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(e != nullptr, OFX_EINVAL, "edge_softmax_csr_heads: NULL input e");
    return EdgeSoftmaxCsrHeads(stream, row_ptr, col_idx, e, nullptr, out, tmp, tmp_bytes,
                               tmp_size_out, 0);
  });
}

extern "C" int ofx_functional_edge_softmax_csr_heads_grad(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* y, const ofx_tensor_desc* dy, ofx_tensor_desc* dx, void* tmp,
    size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(y != nullptr && dy != nullptr, OFX_EINVAL,
                "edge_softmax_csr_heads_grad: NULL input y or dy");
    return EdgeSoftmaxCsrHeads(stream, row_ptr, col_idx, y, dy, dx, tmp, tmp_bytes, tmp_size_out,
                               0);
  });
}

// ---- functional::GatSoftmaxCsrHeads and its gradient functor ------------------------------------
// Ops "gat_softmax_csr_heads" and "gat_softmax_csr_heads_grad"
// (oneflow/user/ops/gat_softmax_heads_op.cpp) through the same op-registry dispatch
// (INTEGRATION.md §13); negative_slope is the ops' double attr.
namespace oneflow {

int GatSoftmaxCsrHeads(void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
                       const ofx_tensor_desc* s_row, const ofx_tensor_desc* s_col,
                       const ofx_tensor_desc* y, const ofx_tensor_desc* dy, double negative_slope,
                       ofx_tensor_desc* out, ofx_tensor_desc* d_row, void* tmp, size_t tmp_bytes,
                       size_t* tmp_size_out, int num_threads) {
  // an earlier launch's loud failure comes back here as OFX_EPLAN (as for spmm_csr)
  if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("gat_softmax_csr_heads");
  const user_op::AttrMap attrs = {{"negative_slope", user_op::AttrBits<double>(negative_slope)}};
  if (dy == nullptr)
    return ToStatus(RunUserOp("gat_softmax_csr_heads",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                               {"s_row", s_row}, {"s_col", s_col}},
                              {{"out", out}}, attrs, stream, tmp, tmp_bytes, tmp_size_out,
                              Placement(), -1, num_threads));
  return ToStatus(RunUserOp("gat_softmax_csr_heads_grad",
                            {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                             {"s_row", s_row}, {"s_col", s_col}, {"y", y}, {"dy", dy}},
                            {{"ds", out}, {"d_row", d_row}}, attrs, stream, tmp, tmp_bytes,
                            tmp_size_out, Placement(), -1, num_threads));
}

}  // namespace oneflow

extern "C" int ofx_functional_gat_softmax_csr_heads(void* stream, const ofx_tensor_desc* row_ptr,
                                                    const ofx_tensor_desc* col_idx,
                                                    const ofx_tensor_desc* s_row,
                                                    const ofx_tensor_desc* s_col,
                                                    double negative_slope, ofx_tensor_desc* out,
                                                    void* tmp, size_t tmp_bytes,
                                                    size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(s_row != nullptr && s_col != nullptr, OFX_EINVAL,
                "gat_softmax_csr_heads: NULL input s_row or s_col");
    return GatSoftmaxCsrHeads(stream, row_ptr, col_idx, s_row, s_col, nullptr, nullptr,
                              negative_slope, out, nullptr, tmp, tmp_bytes, tmp_size_out, 0);
  });
}

extern "C" int ofx_functional_gat_softmax_csr_heads_grad(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* s_row, const ofx_tensor_desc* s_col, const ofx_tensor_desc* y,
    const ofx_tensor_desc* dy, double negative_slope, ofx_tensor_desc* ds, ofx_tensor_desc* d_row,
    void* tmp, size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(s_row != nullptr && s_col != nullptr && y != nullptr && dy != nullptr, OFX_EINVAL,
                "gat_softmax_csr_heads_grad: NULL input s_row, s_col, y or dy");
    return GatSoftmaxCsrHeads(stream, row_ptr, col_idx, s_row, s_col, y, dy, negative_slope, ds,
                              d_row, tmp, tmp_bytes, tmp_size_out, 0);
  });
}

// ---- functional::Gatv2ScoresCsrHeads and its gradient functor -----------------------------------
// Ops "gatv2_scores_csr_heads" and "gatv2_scores_csr_heads_grad"
// (oneflow/user/ops/gatv2_scores_heads_op.cpp) through the same op-registry dispatch
// (INTEGRATION.md §14).
extern "C" int ofx_functional_gatv2_scores_csr_heads(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* x_row, const ofx_tensor_desc* x_col, const ofx_tensor_desc* att,
    int64_t num_heads, double negative_slope, ofx_tensor_desc* out, void* tmp, size_t tmp_bytes,
    size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(x_row != nullptr && x_col != nullptr && att != nullptr, OFX_EINVAL,
                "gatv2_scores_csr_heads: NULL input x_row, x_col or att");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("gatv2_scores_csr_heads");
    return ToStatus(RunUserOp(
        "gatv2_scores_csr_heads",
        {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"x_row", x_row},
         {"x_col", x_col}, {"att", att}},
        {{"out", out}},
        {{"num_heads", num_heads}, {"negative_slope", user_op::AttrBits<double>(negative_slope)}},
        stream, tmp, tmp_bytes, tmp_size_out));
  });
}

extern "C" int ofx_functional_gatv2_scores_csr_heads_grad(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* x_row, const ofx_tensor_desc* x_col, const ofx_tensor_desc* att,
    const ofx_tensor_desc* dy, int64_t num_heads, double negative_slope, int64_t with_att,
    ofx_tensor_desc* d_x, ofx_tensor_desc* p, void* tmp, size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(x_row != nullptr && x_col != nullptr && att != nullptr && dy != nullptr,
                OFX_EINVAL, "gatv2_scores_csr_heads_grad: NULL input x_row, x_col, att or dy");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("gatv2_scores_csr_heads_grad");
    return ToStatus(RunUserOp(
        "gatv2_scores_csr_heads_grad",
        {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"x_row", x_row},
         {"x_col", x_col}, {"att", att}, {"dy", dy}},
        {{"d_x", d_x}, {"p", p}},
        {{"num_heads", num_heads}, {"negative_slope", user_op::AttrBits<double>(negative_slope)},
         {"with_att", with_att != 0 ? 1 : 0}},
        stream, tmp, tmp_bytes, tmp_size_out));
  });
}

// ---- functional::SpmmCsrHeadsFp8 -----------------------------------------------------------------
// Op "spmm_csr_heads_fp8" (oneflow/user/ops/spmm_heads_fp8_op.cpp) through the same op-registry
// dispatch; `b_scale` may be NULL (the optional input is then absent).
extern "C" int ofx_functional_spmm_csr_heads_fp8(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* values, const ofx_tensor_desc* b, const ofx_tensor_desc* b_scale,
    int64_t a_num_rows, int64_t a_num_cols, int64_t b_format, ofx_tensor_desc* out, void* tmp,
    size_t tmp_bytes, size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(values != nullptr && b != nullptr, OFX_EINVAL,
                "spmm_csr_heads_fp8: NULL input a_csr_values or b");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("spmm_csr_heads_fp8");
    std::vector<Arg> ins = {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx},
                            {"a_csr_values", values}, {"b", b}};
    if (b_scale != nullptr) ins.push_back({"b_scale", b_scale});
    return ToStatus(RunUserOp("spmm_csr_heads_fp8", ins, {{"out", out}},
                              {{"a_num_rows", a_num_rows}, {"a_num_cols", a_num_cols},
                               {"b_format", b_format}},
                              stream, tmp, tmp_bytes, tmp_size_out));
  });
}

// ---- functional::GraphAttentionCsrHeads ----------------------------------------------------------
// Op "graph_attention_csr_heads" (oneflow/user/ops/graph_attention_heads_op.cpp) through the same
// op-registry dispatch; two outputs.
extern "C" int ofx_functional_graph_attention_csr_heads(
    void* stream, const ofx_tensor_desc* row_ptr, const ofx_tensor_desc* col_idx,
    const ofx_tensor_desc* q, const ofx_tensor_desc* k, const ofx_tensor_desc* v,
    int64_t num_heads, ofx_tensor_desc* out, ofx_tensor_desc* attn, void* tmp, size_t tmp_bytes,
    size_t* tmp_size_out) {
  return ::ofx::guarded(__func__, [&]() -> int {
    OFX_REQUIRE(q != nullptr && k != nullptr && v != nullptr, OFX_EINVAL,
                "graph_attention_csr_heads: NULL input q, k or v");
    if (tmp_size_out == nullptr) OFX_TAKE_DEVICE_ERROR("graph_attention_csr_heads");
    return ToStatus(RunUserOp("graph_attention_csr_heads",
                              {{"a_csr_row_ptr", row_ptr}, {"a_csr_col_idx", col_idx}, {"q", q},
                               {"k", k}, {"v", v}},
                              {{"out", out}, {"attn", attn}}, {{"num_heads", num_heads}}, stream,
                              tmp, tmp_bytes, tmp_size_out));
  });
}
