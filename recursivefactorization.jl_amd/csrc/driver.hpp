// driver.hpp -- what driver.cpp (handle, schedules, device entries, C ABI) and host_entry.cpp (the host-pointer entries) need from
// each other.  Seen by these two files only.  Templates are instantiated for double and float in the file that defines them.
#pragma once
#include "rflu_internal.hpp"
#include "schedule_plan.hpp"

namespace rflu {

// ---- driver.cpp -------------------------------------------------------------------------------------------------------------------
int64_t workspace_ld(const Handle* h, int64_t n);
SchedIn sched_in(const Handle* h, int64_t m, int64_t n, size_t esize, int pivot, int64_t blocksize, int entry, bool aligned16, int64_t ld);
int get_ustream(Handle* h, int reserve, hipStream_t* out);
int get_pstream(Handle* h, int reserve, hipStream_t* out);
int validate_queues(Handle* h);
int ensure_engine_state(Handle* h);
template <typename T> int getrf_rm(Handle* h, int64_t m, int64_t n, T* R, int64_t ld, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
template <typename T> int getrf_cm_dev(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
template <typename T> int getrs_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb);
template <typename T> int getrs_trans_cm_dev(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb);
template <typename T> int getri_cm_dev(Handle* h, int64_t n, T* F, int64_t lda, const int64_t* ipiv, int64_t* info);

// ---- host_entry.cpp: caller-owned column-major host arrays, staged through device buffers of the handle ---------------------------
template <typename T> int getrf_host(Handle* h, int64_t m, int64_t n, T* A, int64_t lda, int64_t* ipiv, int pivot, int64_t blocksize, int64_t* info);
template <typename T> int getrs_host(Handle* h, int64_t n, int64_t nrhs, const T* F, int64_t lda, const int64_t* ipiv, T* B, int64_t ldb, bool trans);
template <typename T> int getri_host(Handle* h, int64_t n, T* F, int64_t lda, const int64_t* ipiv, int64_t* info);
template <typename T> int logabsdet_host(Handle* h, int64_t n, const T* F, int64_t ld, const int64_t* ipiv, double* logabs, double* sign);

}  // namespace rflu
