// driver.hpp -- what the host sources of librflu.so need from each other: driver.cpp (handle, environment, solves, C ABI), streams.cpp
// (events, masked streams, queue placement), schedule.cpp (the factorization of one matrix on one GPU), mgpu.cpp (multi-GPU) and
// host_entry.cpp (the host-pointer entries).  Seen by these files only.  Templates are instantiated for double and float in the file
// that defines them.
#pragma once
#include "rflu_internal.hpp"
#include "schedule_plan.hpp"

namespace rflu {

// Every API entry runs on the handle's device and leaves the caller's current device as it found it (a framework with
// tensors on several GPUs must not find its current device changed by a library call).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err != hipSuccess) { prev = -1; return; }
        if (prev != dev) err = hipSetDevice(dev);
    }
    // Restores UNCONDITIONALLY: the multi-GPU entry points switch devices inside loops after the guard was taken, so "did the
    // constructor switch?" says nothing about where the current device is when the function returns (or bails out early).
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- driver.cpp -------------------------------------------------------------------------------------------------------------------
const char* env_str(const char* name);   // getenv: for the few measurement switches that are not part of Tune
void load_handle_env(Handle* h);
int64_t workspace_ld(const Handle* h, int64_t n);
template <typename T> int trsm_rec(Handle* h, int64_t n, int64_t nrhs, const T* L, int64_t ldl, T* B, int64_t ldb, const T* linv);
template <typename T> int trsm_public(Handle* h, int64_t n, int64_t nrhs, const T* L, int64_t ldl, T* B, int64_t ldb);
template <typename T> int getrs_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb);
template <typename T> int getrs_trans_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb);
// E: the element trait (rflu_internal.hpp), here and below
template <typename E> int getri_cm_dev(Handle* h, int64_t n, typename E::real* F, int64_t lda, const int64_t* ipiv, int64_t* info);
template <typename T> int gecon_dev(Handle* h, int norm, int64_t n, const T* F, int64_t ld, int row_major, double anorm, double* rcond);

// the argument rules of getri and logabsdet, one copy for the device entries (driver.cpp) and the host entries (host_entry.cpp); the
// latter also leaves the empty product in the outputs.  The sign is one word for real elements, (re, im) for complex ones: sign_im
// belongs to those alone
template <typename E>
inline int getri_check_args(int64_t n, const void* F, int64_t lda, const int64_t* info)
{
    if (n < 0 || lda < (n > 1 ? n : 1) || info == nullptr || (n > 0 && F == nullptr)) {
        set_error("%sgetri: bad arguments n=%lld lda=%lld (or a null pointer)", E::WHO, (long long)n, (long long)lda);
        return RFLU_ERR_ARG;
    }
    return RFLU_OK;
}
template <typename E>
inline int logabsdet_check_args(int64_t n, const void* F, int64_t ld, double* logabs, double* sign_re, double* sign_im)
{
    constexpr bool CPLX = E::PARTS == 2;
    if (n < 0 || ld < (n > 1 ? n : 1) || logabs == nullptr || sign_re == nullptr || (CPLX && sign_im == nullptr) || (n > 0 && F == nullptr)) {
        set_error("%slogabsdet: bad arguments n=%lld ld=%lld (or a null pointer)", E::WHO, (long long)n, (long long)ld);
        return RFLU_ERR_ARG;
    }
    *logabs = 0.0;
    *sign_re = 1.0;
    if (CPLX) *sign_im = 0.0;
    return RFLU_OK;
}

// ---- streams.cpp ------------------------------------------------------------------------------------------------------------------
int get_event(Handle* h, size_t idx, hipEvent_t* ev);   // the handle's reusable events (timing disabled), by number
int get_ustream(Handle* h, int reserve, hipStream_t* out);
int get_pstream(Handle* h, int reserve, hipStream_t* out);
int validate_queues(Handle* h);

// ---- schedule.cpp -----------------------------------------------------------------------------------------------------------------
SchedIn sched_in(const Handle* h, int64_t m, int64_t n, size_t esize, int pivot, int64_t blocksize, int entry, bool aligned16, int64_t ld);
int ensure_engine_state(Handle* h);
int panel_flags_status(Handle* h);   // the error flags the cooperative kernels raise (info_pinned[1]) as a status
template <typename T> int getrf_rm(Handle* h, int64_t m, int64_t n, T* R, int64_t ld, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
template <typename T> int getrf_cm_dev(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
// the Toledo recursion on columns [c0, c0 + w) of an m-row slab, diagonal at (r0, c0), interchanges confined to those columns: enqueued
// on the handle's stream, nothing waited for (mgpu.cpp factors its panels with it); panel_rm is the C ABI's panel entry around it
template <typename T> int panel_rec(Handle* h, int64_t m, int64_t r0, int64_t c0, int64_t w, T* R, int64_t ld, int64_t* ipiv, int pivot);
template <typename T> int panel_rm(Handle* h, int64_t m, int64_t r0, int64_t c0, int64_t w, T* R, int64_t ld, int64_t* ipiv, int pivot, int64_t* info);
template <typename T> int laswp_rm(Handle* h, T* R, int64_t ld, int64_t m, int64_t c0, int64_t ncols, const int64_t* ipiv, int64_t k0, int64_t k1);

// ---- host_entry.cpp: caller-owned column-major host arrays, staged through device buffers of the handle ---------------------------
template <typename T> int getrf_host(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
template <typename T> int getrs_host(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb, bool trans);
// (sign_im: complex elements only)
template <typename E> int getri_host(Handle* h, int64_t n, typename E::real* F, int64_t lda, const int64_t* ipiv, int64_t* info);
template <typename E> int logabsdet_host(Handle* h, int64_t n, const typename E::real* F, int64_t ld, const int64_t* ipiv, double* logabs, double* sign_re, double* sign_im);
template <typename T> int gecon_host(Handle* h, int norm, int64_t n, const T* F, int64_t lda, double anorm, double* rcond);

}  // namespace rflu
