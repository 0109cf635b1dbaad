// Handle lifecycle, options, errors and the RCCL binding of libaiyagari.
#include "internal.h"

#include <cstring>
#include <new>

extern "C" int32_t aiy_version(void) { return 210; }  // 0.2.1: Krusell-Smith employment

// Every handle option once: id, name, field, default and the values it takes.  aiy_set_option,
// aiy_get_option and the handle's defaults all read this table.
namespace {
enum class Takes { flag, range, zero_or_range };   // flag: any nonzero value is 1
struct Option {
  int32_t id;
  const char* name;
  int aiy_handle::*field;
  int def; Takes takes; int64_t lo, hi;
};
#define AIY_FLAG(NAME, field, def) {AIY_OPT_##NAME, "AIY_OPT_" #NAME, &aiy_handle::field, def, Takes::flag, 0, 1}
#define AIY_RANGE(NAME, field, def, lo, hi) {AIY_OPT_##NAME, "AIY_OPT_" #NAME, &aiy_handle::field, def, Takes::range, lo, hi}
const Option kOptions[] = {
    AIY_FLAG(USE_GRAPHS, use_graphs, 1),
    AIY_FLAG(RESIDENT, use_resident, 1),
    AIY_RANGE(RESIDENT_SHAPE, res_shape, 0, 0, 2),
    AIY_FLAG(HIST_FUSED, hist_fused, 0),
    AIY_FLAG(RESIDENT_STREAM, res_stream, 0),
    AIY_FLAG(HIST_RESIDENT, hist_resident, 1),
    AIY_RANGE(HIST_CLUSTER, hist_cluster_cap, 0, 0, 128),
    AIY_RANGE(HIST_ACCEL, hist_accel, 0, 0, 1 << 20),
    AIY_FLAG(HIST_KRYLOV, hist_krylov, 0),
    AIY_FLAG(GE_RESIDENT, ge_resident, 0),
    AIY_RANGE(CU_LIMIT, cu_limit, 0, 0, 65536),
    AIY_RANGE(GE_REBALANCE, ge_rebalance, 55, 0, 100),
    AIY_RANGE(GE_EXTRAP_PERIOD, ge_extrap_period, 32, 4, 1024),
    AIY_RANGE(GE_LOGSEC, ge_logsec, 2, 0, 2),
    AIY_FLAG(HIST_PULL, hist_pull, 0),
    AIY_RANGE(GE_LOOSE_HIST, ge_loose_hist, 8, 6, 14),
    AIY_RANGE(RESIDENT_SHAPE_STREAM, res_shape_stream, 1, -1, 2),
    {AIY_OPT_GE_ANDERSON, "AIY_OPT_GE_ANDERSON", &aiy_handle::ge_anderson, 12, Takes::zero_or_range, 5, 1024},
    AIY_FLAG(HIST_IID, hist_iid, 1),
};
#undef AIY_FLAG
#undef AIY_RANGE

const Option* find_option(aiy_handle* h, int32_t id) {
  for (const Option& o : kOptions)
    if (o.id == id) return &o;
  aiy::fail(h, AIY_ERR_ARG, "unknown option %d", id);
  return nullptr;
}
}  // namespace

aiy_handle::aiy_handle() { for (const Option& o : kOptions) this->*o.field = o.def; }

extern "C" int32_t aiy_set_option(aiy_handle* h, int32_t option, int64_t value) {
  if (!h) return AIY_ERR_ARG;
  const Option* o = find_option(h, option);
  if (!o) return AIY_ERR_ARG;
  if (o->takes == Takes::flag) value = value != 0;
  else if ((value < o->lo || value > o->hi) && !(o->takes == Takes::zero_or_range && value == 0))
    return aiy::fail(h, AIY_ERR_ARG, "%s must be %sin [%lld, %lld]", o->name,
                     o->takes == Takes::zero_or_range ? "0 or " : "", (long long)o->lo, (long long)o->hi);
  h->*o->field = (int)value;
  return AIY_OK;
}

// Current value of a handle option (the values aiy_set_option takes), so callers can save
// and restore what they change.
extern "C" int32_t aiy_get_option(aiy_handle* h, int32_t option, int64_t* value) {
  if (!h || !value) return AIY_ERR_ARG;
  const Option* o = find_option(h, option);
  if (!o) return AIY_ERR_ARG;
  *value = h->*o->field;
  return AIY_OK;
}

extern "C" int32_t aiy_create(int32_t device, aiy_handle** out) {
  if (!out) return AIY_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AIY_ERR_HIP;
  if (device < 0 || device >= n) return AIY_ERR_ARG;
  aiy_handle* h = new (std::nothrow) aiy_handle();
  if (!h) return AIY_ERR_STATE;
  h->device = device;
  if (hipSetDevice(device) != hipSuccess) {
    delete h;
    return AIY_ERR_HIP;
  }
  *out = h;
  return AIY_OK;
}

extern "C" int32_t aiy_destroy(aiy_handle* h) {
  if (!h) return AIY_OK;
  (void)hipSetDevice(h->device);
  if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  delete h;
  return AIY_OK;
}

extern "C" const char* aiy_last_error(const aiy_handle* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int32_t aiy_comm_unique_id(void* out128) {
  if (!out128) return AIY_ERR_ARG;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId must be 128 bytes");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return AIY_ERR_COMM;
  std::memcpy(out128, &id, sizeof(id));
  return AIY_OK;
}

extern "C" int32_t aiy_comm_init(aiy_handle* h, const void* unique_id128, int32_t nranks, int32_t rank) {
  if (!h) return AIY_ERR_ARG;
  if (!unique_id128 || nranks < 1 || rank < 0 || rank >= nranks) return aiy::fail(h, AIY_ERR_ARG, "bad comm args");
  if (h->comm) return aiy::fail(h, AIY_ERR_STATE, "communicator already bound");
  AIY_HIP(h, hipSetDevice(h->device));
  ncclUniqueId id;
  std::memcpy(&id, unique_id128, sizeof(id));
  ncclResult_t r = ncclCommInitRank(&h->comm, nranks, id, rank);
  if (r != ncclSuccess) {
    h->comm = nullptr;
    return aiy::fail(h, AIY_ERR_COMM, "ncclCommInitRank: %s", ncclGetErrorString(r));
  }
  h->nranks = nranks;
  h->rank = rank;
  h->comm_owned = true;
  return AIY_OK;
}

// Borrow a communicator the caller owns (e.g. torch.distributed's RCCL process group, whose
// ncclComm_t ProcessGroupNCCL._comm_ptr() returns): the library enqueues its all-reduces on
// it and never destroys it, so a process keeps ONE communicator per device.  The caller keeps
// it alive until aiy_comm_destroy (which only unbinds it) or aiy_destroy.
extern "C" int32_t aiy_comm_bind(aiy_handle* h, void* comm) {
  if (!h) return AIY_ERR_ARG;
  if (!comm) return aiy::fail(h, AIY_ERR_ARG, "null communicator");
  if (h->comm) return aiy::fail(h, AIY_ERR_STATE, "communicator already bound");
  ncclComm_t c = static_cast<ncclComm_t>(comm);
  int nranks = 0, rank = 0, dev = -1;
  ncclResult_t r = ncclCommCount(c, &nranks);
  if (r == ncclSuccess) r = ncclCommUserRank(c, &rank);
  if (r == ncclSuccess) r = ncclCommCuDevice(c, &dev);
  if (r != ncclSuccess) return aiy::fail(h, AIY_ERR_COMM, "communicator query: %s", ncclGetErrorString(r));
  if (dev != h->device) return aiy::fail(h, AIY_ERR_ARG, "communicator is on device %d, handle on %d", dev, h->device);
  h->comm = c;
  h->comm_owned = false;
  h->nranks = nranks;
  h->rank = rank;
  return AIY_OK;
}

extern "C" int32_t aiy_comm_destroy(aiy_handle* h) {
  if (!h) return AIY_ERR_ARG;
  if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
  h->comm = nullptr;
  h->comm_owned = false;
  h->nranks = 1;
  h->rank = 0;
  return AIY_OK;
}

extern "C" int32_t aiy_allreduce_sum(aiy_handle* h, double* buf, int64_t n, aiy_stream stream) {
  if (!h) return AIY_ERR_ARG;
  if (!h->comm) return aiy::fail(h, AIY_ERR_STATE, "no communicator bound");
  if (!buf || n < 0) return aiy::fail(h, AIY_ERR_ARG, "bad buffer");
  ncclResult_t r = ncclAllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, h->comm, aiy::as_stream(stream));
  if (r != ncclSuccess) return aiy::fail(h, AIY_ERR_COMM, "ncclAllReduce: %s", ncclGetErrorString(r));
  return AIY_OK;
}
