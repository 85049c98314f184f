// loopback_rccl.cpp -- a test-only stand-in for librccl, so that several communicator ranks can share ONE GPU.
//
// Real RCCL refuses two ranks on one device, so the multi-rank lines of shared_simd_scan_amd/csrc/comm.hip (the
// non-root ncclSend, the root's grouped ncclRecv loop, roots other than rank 0, the all-reduce of several counts)
// could otherwise only run on a multi-GPU node.  comm.hip loads the library MI355_RCCL_LIB names with dlopen; pointing
// it at this one makes every rank process talk over abstract-namespace Unix sockets instead, staging device memory
// through the host with hipMemcpyAsync + hipStreamSynchronize on the stream each call was given.
//
// What it checks that real RCCL would not: a receive whose byte count differs from what the peer sent fails with
// ncclInvalidUsage (RCCL would hang or corrupt memory), and every socket has a send / receive timeout, so a missing or
// mismatched peer becomes ncclSystemError instead of a hang.  Built by tests/test_exchange_loopback.py (build_library);
// never linked into, nor loaded by, the product unless MI355_RCCL_LIB names it.
//
// Environment:
//   MI355_LOOPBACK_TIMEOUT_S=<s>   socket timeouts and the mesh deadline (default 60)
//   MI355_LOOPBACK_LOG=<path>      every call appends one line to <path>.<rank>: op, peer, bytes, device pointer,
//                                  stream, group number (0 = outside a group), result
//   MI355_LOOPBACK_FAIL_INIT=<r>   rank r's ncclCommInitRank fails AFTER the mesh is complete (no peer is left waiting)
//   MI355_LOOPBACK_HOST_MEM=1      buffers are host memory and streams are ignored (CPU test of the transport itself)
#include <rccl/rccl.h>

#include <poll.h>
#include <sys/random.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

struct ncclComm {
    int world = 1, rank = 0;
    std::vector<int> fd; // fd[peer]; -1 for this rank itself
};

namespace {

const char kMagic[8] = {'M', 'I', '3', '5', '5', 'L', 'B', '1'};
constexpr uint32_t kWire = 0x4c4f4f50u; // "LOOP": first word of every header on the wire
enum : uint32_t { kOpHello = 1, kOpP2P = 2, kOpAllReduce = 3, kOpError = 4 };

struct Hdr {
    uint32_t wire, op;
    uint64_t bytes; // payload bytes that follow (hello: the sender's rank in the low half, world in the high half)
};

struct Pending {
    bool send;
    const void *sbuf;
    void *rbuf;
    size_t bytes;
    int peer;
    ncclComm *comm;
    hipStream_t stream;
};

// group state is per host thread, as in RCCL
thread_local int t_depth = 0;
thread_local uint64_t t_group = 0;
thread_local std::vector<Pending> t_queue;
std::mutex g_log_mu;
uint64_t g_groups = 0; // groups opened in this process (under g_log_mu)
int g_log_rank = -1;   // rank of the most recent communicator (names the log file of the group calls)

double timeout_s()
{
    const char *e = getenv("MI355_LOOPBACK_TIMEOUT_S");
    double t = e && *e ? atof(e) : 60.0;
    return t > 0 ? t : 60.0;
}

bool host_mem()
{
    const char *e = getenv("MI355_LOOPBACK_HOST_MEM");
    return e && *e == '1';
}

void complain(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void complain(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "loopback_rccl[pid %d]: %s\n", (int)getpid(), buf);
    fflush(stderr);
}

void log_call(int rank, const char *op, int peer, uint64_t bytes, const void *ptr, hipStream_t stream, uint64_t group,
              ncclResult_t rc)
{
    const char *base = getenv("MI355_LOOPBACK_LOG");
    if (!base || !*base) return;
    std::lock_guard<std::mutex> lk(g_log_mu);
    if (rank < 0) rank = g_log_rank;
    std::string path = std::string(base) + "." + std::to_string(rank);
    FILE *f = fopen(path.c_str(), "a");
    if (!f) return;
    fprintf(f, "%s peer=%d bytes=%" PRIu64 " ptr=0x%" PRIxPTR " stream=0x%" PRIxPTR " group=%" PRIu64 " rc=%d\n", op, peer,
            bytes, (uintptr_t)ptr, (uintptr_t)stream, group, (int)rc);
    fclose(f);
}

bool write_all(int fd, const void *p, size_t n, int peer)
{
    const char *c = (const char *)p;
    while (n) {
        ssize_t k = send(fd, c, n, MSG_NOSIGNAL);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) {
            complain("send to rank %d failed: %s", peer,
                     (errno == EAGAIN || errno == EWOULDBLOCK) ? "timed out (peer not receiving)" : strerror(errno));
            return false;
        }
        c += k;
        n -= (size_t)k;
    }
    return true;
}

bool read_all(int fd, void *p, size_t n, int peer)
{
    char *c = (char *)p;
    while (n) {
        ssize_t k = recv(fd, c, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) {
            complain("receive from rank %d failed: %s", peer,
                     k == 0 ? "peer closed the connection"
                            : (errno == EAGAIN || errno == EWOULDBLOCK) ? "timed out (peer not sending)" : strerror(errno));
            return false;
        }
        c += k;
        n -= (size_t)k;
    }
    return true;
}

bool drain(int fd, uint64_t n, int peer)
{
    char tmp[1 << 14];
    while (n) {
        size_t k = n < sizeof tmp ? (size_t)n : sizeof tmp;
        if (!read_all(fd, tmp, k, peer)) return false;
        n -= k;
    }
    return true;
}

void set_timeouts(int fd)
{
    double t = timeout_s();
    timeval tv;
    tv.tv_sec = (time_t)t;
    tv.tv_usec = (suseconds_t)((t - (double)tv.tv_sec) * 1e6);
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof tv);
}

socklen_t address(const ncclUniqueId &id, int rank, sockaddr_un *a)
{
    // abstract namespace (leading NUL): nothing on the file system, gone when the last socket closes
    memset(a, 0, sizeof *a);
    a->sun_family = AF_UNIX;
    char name[96];
    int k = snprintf(name, sizeof name, "mi355-loopback-");
    for (int i = 0; i < 16; i++) k += snprintf(name + k, sizeof name - k, "%02x", (unsigned char)id.internal[8 + i]);
    k += snprintf(name + k, sizeof name - k, "-%d", rank);
    memcpy(a->sun_path + 1, name, (size_t)k);
    return (socklen_t)(offsetof(sockaddr_un, sun_path) + 1 + k);
}

void close_all(ncclComm *c)
{
    for (int &f : c->fd)
        if (f >= 0) {
            close(f);
            f = -1;
        }
}

ncclResult_t hip_err(hipError_t e, const char *what)
{
    complain("%s: %s", what, hipGetErrorString(e));
    return ncclUnhandledCudaError;
}

// device <-> host staging, ordered on the call's stream: everything enqueued before the call has finished when the
// copy runs, and the copy has finished when the call returns
ncclResult_t to_host(void *dst, const void *src, size_t n, hipStream_t s)
{
    if (!n) return ncclSuccess;
    if (host_mem()) {
        memcpy(dst, src, n);
        return ncclSuccess;
    }
    hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? ncclSuccess : hip_err(e, "device -> host copy");
}

ncclResult_t to_device(void *dst, const void *src, size_t n, hipStream_t s)
{
    if (!n) return ncclSuccess;
    if (host_mem()) {
        memcpy(dst, src, n);
        return ncclSuccess;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? ncclSuccess : hip_err(e, "host -> device copy");
}

bool peer_ok(const ncclComm *c, int peer) { return c && peer >= 0 && peer < c->world && peer != c->rank && c->fd[peer] >= 0; }

ncclResult_t do_send(const Pending &p)
{
    std::vector<uint8_t> host(p.bytes);
    ncclResult_t r = to_host(host.data(), p.sbuf, p.bytes, p.stream);
    if (r != ncclSuccess) return r;
    Hdr h{kWire, kOpP2P, p.bytes};
    int fd = p.comm->fd[p.peer];
    if (!write_all(fd, &h, sizeof h, p.peer) || !write_all(fd, host.data(), host.size(), p.peer)) return ncclSystemError;
    return ncclSuccess;
}

ncclResult_t do_recv(const Pending &p)
{
    Hdr h;
    int fd = p.comm->fd[p.peer];
    if (!read_all(fd, &h, sizeof h, p.peer)) return ncclSystemError;
    if (h.wire != kWire || h.op != kOpP2P) {
        complain("rank %d: ncclRecv from rank %d met a message of another kind (op %u)", p.comm->rank, p.peer, h.op);
        return ncclInvalidUsage;
    }
    if (h.bytes != p.bytes) {
        complain("rank %d: ncclRecv of %zu bytes from rank %d, which sent %" PRIu64 " bytes", p.comm->rank, p.bytes, p.peer,
                 h.bytes);
        drain(fd, h.bytes, p.peer); // keep the channel in step; the call fails either way
        return ncclInvalidUsage;
    }
    std::vector<uint8_t> host(p.bytes);
    if (!read_all(fd, host.data(), host.size(), p.peer)) return ncclSystemError;
    return to_device(p.rbuf, host.data(), p.bytes, p.stream);
}

size_t p2p_bytes(size_t count, ncclDataType_t t) { return (t == ncclUint8 || t == ncclInt8) ? count : (size_t)-1; }

ncclResult_t post(bool send, const void *sbuf, void *rbuf, size_t count, ncclDataType_t t, int peer, ncclComm *comm,
                  hipStream_t stream)
{
    const char *op = send ? "ncclSend" : "ncclRecv";
    const size_t bytes = p2p_bytes(count, t);
    ncclResult_t rc = ncclSuccess;
    if (!comm)
        rc = ncclInvalidArgument;
    else if (bytes == (size_t)-1) {
        complain("%s: only ncclUint8 / ncclInt8 are supported (datatype %d)", op, (int)t);
        rc = ncclInvalidArgument;
    } else if (!peer_ok(comm, peer)) {
        complain("%s: peer %d is not another rank of a world of %d", op, peer, comm->world);
        rc = ncclInvalidArgument;
    } else if (bytes && !(send ? sbuf : rbuf)) {
        rc = ncclInvalidArgument;
    }
    Pending p{send, sbuf, rbuf, bytes, peer, comm, stream};
    if (rc == ncclSuccess && bytes) {
        if (t_depth > 0)
            t_queue.push_back(p); // runs in ncclGroupEnd
        else
            rc = send ? do_send(p) : do_recv(p);
    }
    log_call(comm ? comm->rank : -1, op, peer, bytes, send ? sbuf : rbuf, stream, t_depth > 0 ? t_group : 0, rc);
    return rc;
}

} // namespace

extern "C" {

const char *ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error (loopback)";
    case ncclUnhandledCudaError: return "unhandled HIP error (loopback)";
    case ncclSystemError: return "system error: peer missing, closed or timed out (loopback)";
    case ncclInternalError: return "internal error (loopback)";
    case ncclInvalidArgument: return "invalid argument (loopback)";
    case ncclInvalidUsage: return "invalid usage: mismatched send / receive (loopback)";
    case ncclRemoteError: return "remote error (loopback)";
    case ncclInProgress: return "in progress (loopback)";
    default: return "unknown result (loopback)";
    }
}

ncclResult_t ncclGetUniqueId(ncclUniqueId *id)
{
    if (!id) return ncclInvalidArgument;
    memset(id, 0, sizeof *id);
    memcpy(id->internal, kMagic, sizeof kMagic);
    if (getrandom(id->internal + 8, 16, 0) != 16) {
        complain("getrandom: %s", strerror(errno));
        return ncclSystemError;
    }
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *out, int nranks, ncclUniqueId id, int rank)
{
    if (!out || nranks < 1 || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    if (memcmp(id.internal, kMagic, sizeof kMagic) != 0) {
        complain("ncclCommInitRank: the unique id was not made by this library");
        return ncclInvalidArgument;
    }
    {
        std::lock_guard<std::mutex> lk(g_log_mu);
        g_log_rank = rank;
    }
    ncclComm *c = new ncclComm;
    c->world = nranks;
    c->rank = rank;
    c->fd.assign(nranks, -1);
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s());
    auto left_ms = [&] {
        auto d = std::chrono::duration_cast<std::chrono::milliseconds>(deadline - std::chrono::steady_clock::now()).count();
        return d > 0 ? (int)d : 0;
    };
    ncclResult_t rc = ncclSuccess;
    int lfd = -1;
    // full mesh: listen on this rank's name, connect to every lower rank, accept every higher one.  Connecting needs
    // only the peer's listen backlog, not its accept, so the order cannot deadlock.
    if (nranks > 1) {
        sockaddr_un a;
        socklen_t al = address(id, rank, &a);
        lfd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
        if (lfd < 0 || bind(lfd, (sockaddr *)&a, al) != 0 || listen(lfd, nranks) != 0) {
            complain("rank %d: cannot listen: %s", rank, strerror(errno));
            rc = ncclSystemError;
        }
        for (int p = 0; rc == ncclSuccess && p < rank; p++) {
            socklen_t pl = address(id, p, &a);
            int s = -1;
            while (true) {
                s = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
                if (s >= 0 && connect(s, (sockaddr *)&a, pl) == 0) break;
                if (s >= 0) close(s);
                s = -1;
                if (!left_ms()) break;
                std::this_thread::sleep_for(std::chrono::milliseconds(10));
            }
            if (s < 0) {
                complain("rank %d: rank %d never listened (deadline %.0f s)", rank, p, timeout_s());
                rc = ncclSystemError;
                break;
            }
            set_timeouts(s);
            c->fd[p] = s;
            Hdr h{kWire, kOpHello, (uint64_t)rank | ((uint64_t)nranks << 32)}, ack;
            if (!write_all(s, &h, sizeof h, p) || !read_all(s, &ack, sizeof ack, p)) {
                rc = ncclSystemError;
            } else if (ack.wire != kWire || ack.op != kOpHello || ack.bytes != ((uint64_t)p | ((uint64_t)nranks << 32))) {
                complain("rank %d: rank %d answered for another world (wanted rank %d of %d)", rank, p, p, nranks);
                rc = ncclSystemError;
            }
        }
        for (int k = rank + 1; rc == ncclSuccess && k < nranks; k++) {
            pollfd pf{lfd, POLLIN, 0};
            int pr = poll(&pf, 1, left_ms());
            if (pr < 0 && errno == EINTR) {
                k--;
                continue;
            }
            int s = pr > 0 ? accept4(lfd, nullptr, nullptr, SOCK_CLOEXEC) : -1;
            if (s < 0) {
                complain("rank %d: %d higher rank(s) never connected (deadline %.0f s)", rank, nranks - k, timeout_s());
                rc = ncclSystemError;
                break;
            }
            set_timeouts(s);
            Hdr h;
            if (!read_all(s, &h, sizeof h, -1)) {
                close(s);
                rc = ncclSystemError;
                break;
            }
            const int peer = (int)(uint32_t)h.bytes, pw = (int)(h.bytes >> 32);
            if (h.wire != kWire || h.op != kOpHello || pw != nranks || peer <= rank || peer >= nranks || c->fd[peer] >= 0) {
                complain("rank %d: bad hello (rank %d of a world of %d)", rank, peer, pw);
                close(s);
                rc = ncclSystemError;
                break;
            }
            c->fd[peer] = s;
            Hdr ack{kWire, kOpHello, (uint64_t)rank | ((uint64_t)nranks << 32)};
            if (!write_all(s, &ack, sizeof ack, peer)) rc = ncclSystemError;
        }
        if (lfd >= 0) close(lfd);
    }
    const char *fi = getenv("MI355_LOOPBACK_FAIL_INIT");
    if (rc == ncclSuccess && fi && *fi && atoi(fi) == rank) {
        complain("rank %d: ncclCommInitRank fails on purpose (MI355_LOOPBACK_FAIL_INIT)", rank);
        rc = ncclSystemError;
    }
    if (rc != ncclSuccess) {
        close_all(c);
        delete c;
        c = nullptr;
    }
    *out = c;
    log_call(rank, "ncclCommInitRank", -1, 0, nullptr, nullptr, 0, rc);
    return rc;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    if (!comm) return ncclInvalidArgument;
    log_call(comm->rank, "ncclCommDestroy", -1, 0, nullptr, nullptr, 0, ncclSuccess);
    close_all(comm);
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclGroupStart()
{
    if (t_depth++ == 0) {
        std::lock_guard<std::mutex> lk(g_log_mu);
        t_group = ++g_groups;
        t_queue.clear();
    }
    log_call(-1, "ncclGroupStart", -1, 0, nullptr, nullptr, t_group, ncclSuccess);
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    if (t_depth <= 0) return ncclInvalidUsage;
    ncclResult_t rc = ncclSuccess;
    const uint64_t g = t_group;
    if (--t_depth == 0) {
        // every send first, then every receive: a rank that both sends and receives never waits on a peer that is itself
        // waiting to send (sends only block once a socket buffer is full, until the peer reads)
        std::vector<Pending> q;
        q.swap(t_queue);
        for (int pass = 0; pass < 2 && rc == ncclSuccess; pass++)
            for (const Pending &p : q)
                if (p.send == (pass == 0) && rc == ncclSuccess) rc = p.send ? do_send(p) : do_recv(p);
        t_group = 0;
    }
    log_call(-1, "ncclGroupEnd", -1, 0, nullptr, nullptr, g, rc);
    return rc;
}

ncclResult_t ncclSend(const void *sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream)
{
    return post(true, sendbuff, nullptr, count, datatype, peer, comm, stream);
}

ncclResult_t ncclRecv(void *recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream)
{
    return post(false, nullptr, recvbuff, count, datatype, peer, comm, stream);
}

ncclResult_t ncclAllReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op,
                           ncclComm_t comm, hipStream_t stream)
{
    // sum of 64-bit integers only (what comm.hip asks for): gathered on rank 0, added with uint64 wrap-around (the
    // same bits for int64), sent back; in place (sendbuff == recvbuff) allowed
    const size_t bytes = count * 8;
    ncclResult_t rc = ncclSuccess;
    if (!comm || (count && (!sendbuff || !recvbuff))) {
        rc = ncclInvalidArgument;
    } else if ((datatype != ncclUint64 && datatype != ncclInt64) || op != ncclSum) {
        complain("ncclAllReduce: only ncclSum over ncclUint64 / ncclInt64 is supported (datatype %d, op %d)", (int)datatype,
                 (int)op);
        rc = ncclInvalidArgument;
    } else if (t_depth > 0) {
        complain("ncclAllReduce inside a group is not supported");
        rc = ncclInvalidUsage;
    }
    std::vector<uint64_t> acc(count), tmp(count);
    if (rc == ncclSuccess) rc = to_host(acc.data(), sendbuff, bytes, stream);
    if (rc == ncclSuccess && comm->world > 1) {
        if (comm->rank == 0) {
            ncclResult_t bad = ncclSuccess; // a peer with another count: every peer is told, none is left waiting
            for (int p = 1; p < comm->world && rc == ncclSuccess; p++) {
                Hdr h;
                if (!read_all(comm->fd[p], &h, sizeof h, p)) {
                    rc = ncclSystemError;
                } else if (h.wire != kWire || h.op != kOpAllReduce || h.bytes != bytes) {
                    complain("rank 0: ncclAllReduce of %zu bytes, rank %d contributed op %u with %" PRIu64 " bytes", bytes, p,
                             h.op, h.bytes);
                    if (!drain(comm->fd[p], h.bytes, p)) rc = ncclSystemError;
                    bad = ncclInvalidUsage;
                } else if (!read_all(comm->fd[p], tmp.data(), bytes, p)) {
                    rc = ncclSystemError;
                } else {
                    for (size_t i = 0; i < count; i++) acc[i] += tmp[i];
                }
            }
            if (rc == ncclSuccess) rc = bad;
            Hdr back{kWire, rc == ncclSuccess ? (uint32_t)kOpAllReduce : (uint32_t)kOpError, rc == ncclSuccess ? bytes : 0};
            for (int p = 1; p < comm->world; p++)
                if (!write_all(comm->fd[p], &back, sizeof back, p) ||
                    (rc == ncclSuccess && !write_all(comm->fd[p], acc.data(), bytes, p)))
                    rc = ncclSystemError;
        } else {
            Hdr h{kWire, kOpAllReduce, bytes}, back;
            if (!write_all(comm->fd[0], &h, sizeof h, 0) || !write_all(comm->fd[0], acc.data(), bytes, 0) ||
                !read_all(comm->fd[0], &back, sizeof back, 0)) {
                rc = ncclSystemError;
            } else if (back.wire != kWire || back.op != kOpAllReduce || back.bytes != bytes) {
                complain("rank %d: ncclAllReduce refused by rank 0 (the ranks disagree on the count)", comm->rank);
                if (back.op == kOpAllReduce) drain(comm->fd[0], back.bytes, 0);
                rc = ncclInvalidUsage;
            } else if (!read_all(comm->fd[0], acc.data(), bytes, 0)) {
                rc = ncclSystemError;
            }
        }
    }
    if (rc == ncclSuccess) rc = to_device(recvbuff, acc.data(), bytes, stream);
    log_call(comm ? comm->rank : -1, "ncclAllReduce", -1, bytes, recvbuff, stream, 0, rc);
    return rc;
}

} // extern "C"
