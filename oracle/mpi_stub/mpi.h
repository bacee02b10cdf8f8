/* A one-rank MPI, header only: just enough of the MPI C binding (signatures as
 * in the MPI 3.1 standard) to run a Cartesian halo-exchange program as a
 * single process.  World size 1, rank 0, a 1 x 1 process grid, every
 * Cartesian neighbour MPI_PROC_NULL.  Communication with MPI_PROC_NULL does
 * nothing, as the standard defines; any call that would have to reach a real
 * peer aborts with a message instead of pretending.
 *
 * It exists to build reference binaries for comparisons (oracle/build_ref.py);
 * nothing of the product links against it. */
#ifndef ORACLE_MPI_STUB_H
#define ORACLE_MPI_STUB_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

/* The recorded results are those of strict IEEE evaluation: float expressions
 * in float, double expressions in double (SSE2, not x87 extended precision). */
#if defined(__FLT_EVAL_METHOD__) && __FLT_EVAL_METHOD__ != 0
#error "the reference binaries need FLT_EVAL_METHOD 0 (build with SSE arithmetic)"
#endif

typedef int MPI_Comm;
typedef int MPI_Datatype;
typedef int MPI_Op;
typedef int MPI_Request;
typedef struct MPI_Status {
  int MPI_SOURCE, MPI_TAG, MPI_ERROR;
} MPI_Status;

#define MPI_SUCCESS 0
#define MPI_COMM_WORLD ((MPI_Comm)1)
#define MPI_PROC_NULL (-2)
#define MPI_ANY_SOURCE (-1)
#define MPI_ANY_TAG (-1)
#define MPI_REQUEST_NULL ((MPI_Request)0)
#define MPI_STATUS_IGNORE ((MPI_Status*)0)
#define MPI_STATUSES_IGNORE ((MPI_Status*)0)

#define MPI_INT ((MPI_Datatype)1)
#define MPI_FLOAT ((MPI_Datatype)2)
#define MPI_DOUBLE ((MPI_Datatype)3)
#define MPI_STUB_DERIVED ((MPI_Datatype)100) /* contiguous / vector types: never moved */

#define MPI_LAND ((MPI_Op)1)
#define MPI_MAX ((MPI_Op)2)
#define MPI_MIN ((MPI_Op)3)
#define MPI_SUM ((MPI_Op)4)

/* A persistent request to MPI_PROC_NULL; the only kind there is here. */
#define MPI_STUB_NULL_PEER_REQUEST ((MPI_Request)7)

static void mpi_stub_die(const char* call, const char* why) {
  fprintf(stderr, "mpi stub: %s: %s (this MPI has one rank and no peers)\n", call, why);
  fflush(NULL);
  abort();
}

static size_t mpi_stub_sizeof(const char* call, MPI_Datatype t) {
  switch (t) {
    case MPI_INT: return sizeof(int);
    case MPI_FLOAT: return sizeof(float);
    case MPI_DOUBLE: return sizeof(double);
    default: mpi_stub_die(call, "datatype without a known size"); return 0;
  }
}

static inline int MPI_Init(int* argc, char*** argv) {
  (void)argc; (void)argv;
  return MPI_SUCCESS;
}

static inline int MPI_Finalize(void) { return MPI_SUCCESS; }

static inline double MPI_Wtime(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static inline int MPI_Comm_size(MPI_Comm comm, int* size) {
  (void)comm;
  *size = 1;
  return MPI_SUCCESS;
}

static inline int MPI_Comm_rank(MPI_Comm comm, int* rank) {
  (void)comm;
  *rank = 0;
  return MPI_SUCCESS;
}

/* One node: every dimension left free (0) becomes 1; a fixed one must be 1. */
static inline int MPI_Dims_create(int nnodes, int ndims, int dims[]) {
  int d;
  if (nnodes != 1) mpi_stub_die("MPI_Dims_create", "more than one node");
  for (d = 0; d < ndims; ++d) {
    if (dims[d] == 0) dims[d] = 1;
    else if (dims[d] != 1) mpi_stub_die("MPI_Dims_create", "a fixed dimension other than 1");
  }
  return MPI_SUCCESS;
}

static inline int MPI_Cart_create(MPI_Comm comm_old, int ndims, const int dims[],
                                  const int periods[], int reorder, MPI_Comm* comm_cart) {
  int d;
  (void)comm_old; (void)reorder;
  for (d = 0; d < ndims; ++d) {
    if (dims[d] != 1) mpi_stub_die("MPI_Cart_create", "a process grid larger than 1 x 1");
    if (periods[d]) mpi_stub_die("MPI_Cart_create", "a periodic grid (a rank would be its own peer)");
  }
  *comm_cart = (MPI_Comm)2;
  return MPI_SUCCESS;
}

static inline int MPI_Cart_coords(MPI_Comm comm, int rank, int maxdims, int coords[]) {
  int d;
  (void)comm;
  if (rank != 0) mpi_stub_die("MPI_Cart_coords", "a rank other than 0");
  for (d = 0; d < maxdims; ++d) coords[d] = 0;
  return MPI_SUCCESS;
}

/* Non-periodic 1 x 1 grid: any non-zero shift runs off the grid on both sides. */
static inline int MPI_Cart_shift(MPI_Comm comm, int direction, int disp, int* rank_source,
                                 int* rank_dest) {
  (void)comm; (void)direction;
  *rank_source = *rank_dest = disp == 0 ? 0 : MPI_PROC_NULL;
  return MPI_SUCCESS;
}

static inline int MPI_Type_contiguous(int count, MPI_Datatype oldtype, MPI_Datatype* newtype) {
  (void)count; (void)oldtype;
  *newtype = MPI_STUB_DERIVED;
  return MPI_SUCCESS;
}

static inline int MPI_Type_vector(int count, int blocklength, int stride, MPI_Datatype oldtype,
                                  MPI_Datatype* newtype) {
  (void)count; (void)blocklength; (void)stride; (void)oldtype;
  *newtype = MPI_STUB_DERIVED;
  return MPI_SUCCESS;
}

static inline int MPI_Type_commit(MPI_Datatype* datatype) {
  (void)datatype;
  return MPI_SUCCESS;
}

static inline int MPI_Send(const void* buf, int count, MPI_Datatype datatype, int dest, int tag,
                           MPI_Comm comm) {
  (void)buf; (void)count; (void)datatype; (void)tag; (void)comm;
  if (dest != MPI_PROC_NULL) mpi_stub_die("MPI_Send", "a send to a real rank");
  return MPI_SUCCESS;
}

static inline int MPI_Recv(void* buf, int count, MPI_Datatype datatype, int source, int tag,
                           MPI_Comm comm, MPI_Status* status) {
  (void)buf; (void)count; (void)datatype; (void)tag; (void)comm;
  if (source != MPI_PROC_NULL) mpi_stub_die("MPI_Recv", "a receive from a real rank");
  if (status != MPI_STATUS_IGNORE) {
    status->MPI_SOURCE = MPI_PROC_NULL;
    status->MPI_TAG = MPI_ANY_TAG;
    status->MPI_ERROR = MPI_SUCCESS;
  }
  return MPI_SUCCESS;
}

static inline int MPI_Send_init(const void* buf, int count, MPI_Datatype datatype, int dest,
                                int tag, MPI_Comm comm, MPI_Request* request) {
  (void)buf; (void)count; (void)datatype; (void)tag; (void)comm;
  if (dest != MPI_PROC_NULL) mpi_stub_die("MPI_Send_init", "a persistent send to a real rank");
  *request = MPI_STUB_NULL_PEER_REQUEST;
  return MPI_SUCCESS;
}

static inline int MPI_Recv_init(void* buf, int count, MPI_Datatype datatype, int source, int tag,
                                MPI_Comm comm, MPI_Request* request) {
  (void)buf; (void)count; (void)datatype; (void)tag; (void)comm;
  if (source != MPI_PROC_NULL) mpi_stub_die("MPI_Recv_init", "a persistent receive from a real rank");
  *request = MPI_STUB_NULL_PEER_REQUEST;
  return MPI_SUCCESS;
}

static inline int MPI_Startall(int count, MPI_Request array_of_requests[]) {
  int i;
  for (i = 0; i < count; ++i)
    if (array_of_requests[i] != MPI_STUB_NULL_PEER_REQUEST)
      mpi_stub_die("MPI_Startall", "a request that no *_init of this MPI made");
  return MPI_SUCCESS;
}

static inline int MPI_Waitall(int count, MPI_Request array_of_requests[],
                              MPI_Status array_of_statuses[]) {
  int i;
  (void)array_of_statuses;
  for (i = 0; i < count; ++i)
    if (array_of_requests[i] != MPI_STUB_NULL_PEER_REQUEST &&
        array_of_requests[i] != MPI_REQUEST_NULL)
      mpi_stub_die("MPI_Waitall", "a request that no *_init of this MPI made");
  return MPI_SUCCESS;
}

static inline int MPI_Request_free(MPI_Request* request) {
  *request = MPI_REQUEST_NULL;
  return MPI_SUCCESS;
}

/* One rank: every reduction of one contribution is that contribution. */
static inline int MPI_Allreduce(const void* sendbuf, void* recvbuf, int count,
                                MPI_Datatype datatype, MPI_Op op, MPI_Comm comm) {
  (void)op; (void)comm;
  memcpy(recvbuf, sendbuf, (size_t)count * mpi_stub_sizeof("MPI_Allreduce", datatype));
  return MPI_SUCCESS;
}

#endif /* ORACLE_MPI_STUB_H */
