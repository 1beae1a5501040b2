// Native DevicePlugin v1beta1 gRPC server (C++ / nghttp2 over a unix socket).
//
// The reference's runtime is a compiled Go daemon; this is the MI355X
// build's native equivalent for the kubelet-facing hot path.  Python owns
// discovery/health/lifecycle and pushes PRE-SERIALIZED state (device list
// bytes, per-device Allocate fragments, allocator tables); this server
// owns the wire: HTTP/2 via the system libnghttp2 (dlopen, nghttp2_abi.h),
// gRPC framing, request parsing and the preferred-allocation search
// (pref_alloc.h) — no Python in the request path, so Allocate latency is
// the kernel's UDS round trip plus microseconds of C++.
//
// Protocol surface (identical to the Python grpc server, conformance-tested
// against the Python grpc client in tests/test_fastserver.py):
//   /v1beta1.DevicePlugin/GetDevicePluginOptions   unary, fixed bytes
//   /v1beta1.DevicePlugin/PreStartContainer        unary, empty
//   /v1beta1.DevicePlugin/Allocate                 unary, assembled reply
//   /v1beta1.DevicePlugin/GetPreferredAllocation   unary, native search
//   /v1beta1.DevicePlugin/ListAndWatch             server-streaming + pushes

#include <arpa/inet.h>
#include <errno.h>
#include <fcntl.h>
#include <poll.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "nghttp2_abi.h"
#include "pref_alloc.h"

namespace py = pybind11;
using prefalloc::AllocState;
using prefalloc::preferred_alloc;

namespace {

// ---------------- protobuf wire helpers ----------------

void put_varint(std::string &out, uint64_t v) {
    while (v >= 0x80) {
        out.push_back((char)(v | 0x80));
        v >>= 7;
    }
    out.push_back((char)v);
}

bool get_varint(const uint8_t *&p, const uint8_t *end, uint64_t &v) {
    v = 0;
    int shift = 0;
    while (p < end && shift < 64) {
        uint8_t b = *p++;
        v |= (uint64_t)(b & 0x7F) << shift;
        if (!(b & 0x80)) return true;
        shift += 7;
    }
    return false;
}

void put_len_delim(std::string &out, int field, const std::string &bytes) {
    put_varint(out, (uint64_t)(field << 3) | 2);
    put_varint(out, bytes.size());
    out += bytes;
}

// Iterate fields of a serialized message; cb(field_no, wire_type, ptr, len_or_varint)
template <typename F>
bool for_each_field(const uint8_t *p, const uint8_t *end, F cb) {
    while (p < end) {
        uint64_t key;
        if (!get_varint(p, end, key)) return false;
        int field = (int)(key >> 3), wt = (int)(key & 7);
        if (wt == 0) {  // varint
            uint64_t v;
            if (!get_varint(p, end, v)) return false;
            cb(field, wt, (const uint8_t *)nullptr, v);
        } else if (wt == 2) {  // len-delim
            uint64_t len;
            if (!get_varint(p, end, len)) return false;
            if ((uint64_t)(end - p) < len) return false;
            cb(field, wt, p, len);
            p += len;
        } else if (wt == 5) {
            if (end - p < 4) return false;
            p += 4;
        } else if (wt == 1) {
            if (end - p < 8) return false;
            p += 8;
        } else {
            return false;
        }
    }
    return true;
}

// ---------------- gRPC framing ----------------

constexpr size_t kGrpcPrefix = 5;  // compressed flag + big-endian length

std::string grpc_frame(const std::string &msg) {
    std::string out;
    out.reserve(msg.size() + kGrpcPrefix);
    out.push_back('\0');
    uint32_t n = htonl((uint32_t)msg.size());
    out.append((const char *)&n, 4);
    out += msg;
    return out;
}

// A unary response is assembled behind kGrpcPrefix placeholder bytes and
// framed in place, so the message is never copied into its frame.
void grpc_frame_in_place(std::string &framed) {
    framed[0] = '\0';
    uint32_t n = htonl((uint32_t)(framed.size() - kGrpcPrefix));
    memcpy(&framed[1], &n, 4);
}

// ---------------- server ----------------

struct Conn;

struct Stream {
    std::string path;
    std::string req_body;
    // outgoing byte queue for the data provider
    std::string out;
    size_t out_off = 0;
    bool is_listwatch = false;
    bool trailer_sent = false;
    std::string grpc_status = "0";
    std::string grpc_message;
    Conn *conn = nullptr;
};

class Server;

struct Conn {
    int fd = -1;
    nghttp2_session *session = nullptr;
    std::map<int32_t, std::unique_ptr<Stream>> streams;
    // Outgoing bytes: what the session had ready, gathered so that one
    // write() sends it; [woff, size) is what the socket has not taken yet.
    std::string wbuf;
    size_t woff = 0;
    bool want_out() const { return woff < wbuf.size(); }
    Server *srv = nullptr;
    bool dead = false;
};

class Server {
  public:
    explicit Server(std::string socket_path) : path_(std::move(socket_path)) {}
    ~Server() { stop(); }

    // ---- state pushed from Python (all pre-serialized protobuf) ----
    void set_options_response(py::bytes b) {
        std::lock_guard<std::mutex> g(mu_);
        options_ = std::string(b);
    }
    void set_kfd_spec(py::bytes b) {
        std::lock_guard<std::mutex> g(mu_);
        kfd_spec_ = std::string(b);
    }
    void set_device_specs(const std::map<std::string, py::bytes> &specs) {
        std::lock_guard<std::mutex> g(mu_);
        dev_specs_.clear();
        for (auto &kv : specs) dev_specs_[kv.first] = std::string(kv.second);
    }
    void set_list_response(py::bytes b) {
        std::lock_guard<std::mutex> g(mu_);
        list_bytes_ = std::string(b);
    }
    void push_list_update(py::bytes b) {
        {
            std::lock_guard<std::mutex> g(mu_);
            list_bytes_ = std::string(b);
            pending_push_ = true;
        }
        wake();
    }
    void set_prestart_paths(const std::map<std::string, std::string> &paths) {
        std::lock_guard<std::mutex> g(mu_);
        prestart_paths_.clear();
        for (auto &kv : paths) prestart_paths_[kv.first] = kv.second;
    }

    py::dict stats() {
        py::dict d;
        d["allocate_total"] = (uint64_t)n_allocate_.load();
        d["preferred_allocation_total"] = (uint64_t)n_preferred_.load();
        d["list_and_watch_streams_total"] = (uint64_t)n_listwatch_.load();
        d["options_total"] = (uint64_t)n_options_.load();
        d["prestart_total"] = (uint64_t)n_prestart_.load();
        d["unknown_method_total"] = (uint64_t)n_unknown_.load();
        d["list_pushes_total"] = (uint64_t)n_pushes_.load();
        d["connections_total"] = (uint64_t)n_conns_.load();
        // handler-time sums (ns): with the *_total counters these give
        // Prometheus-style average handler latency via rate()/rate()
        d["allocate_handler_ns_total"] = (uint64_t)allocate_ns_.load();
        d["preferred_handler_ns_total"] = (uint64_t)preferred_ns_.load();
        // transport: write()/read() calls on kubelet connections, and how
        // often the socket took less than it was offered (back-pressure)
        d["socket_writes_total"] = (uint64_t)n_writes_.load();
        d["socket_reads_total"] = (uint64_t)n_reads_.load();
        d["socket_write_would_block_total"] = (uint64_t)n_would_block_.load();
        return d;
    }

    void set_allocator_state(
        const std::vector<std::pair<std::string, std::vector<int>>> &groups,
        const std::map<std::string, int> &node_of_id,
        const std::vector<std::tuple<int, int, int>> &weights) {
        std::lock_guard<std::mutex> g(mu_);
        alloc_.load(groups, node_of_id, weights);
    }

    void start() {
        if (running_.exchange(true)) return;
        ::unlink(path_.c_str());
        listen_fd_ = ::socket(AF_UNIX, SOCK_STREAM | SOCK_NONBLOCK, 0);
        if (listen_fd_ < 0) throw std::runtime_error("socket() failed");
        sockaddr_un addr{};
        addr.sun_family = AF_UNIX;
        if (path_.size() >= sizeof(addr.sun_path))
            throw std::runtime_error("socket path too long");
        strncpy(addr.sun_path, path_.c_str(), sizeof(addr.sun_path) - 1);
        if (::bind(listen_fd_, (sockaddr *)&addr, sizeof(addr)) != 0)
            throw std::runtime_error("bind() failed: " +
                                     std::string(strerror(errno)));
        if (::listen(listen_fd_, 16) != 0)
            throw std::runtime_error("listen() failed");
        if (::pipe2(wake_pipe_, O_NONBLOCK) != 0)
            throw std::runtime_error("pipe2() failed");
        loop_ = std::thread([this] { run_loop(); });
    }

    void stop() {
        if (!running_.exchange(false)) return;
        wake();
        if (loop_.joinable()) loop_.join();
        for (auto &c : conns_) destroy_conn(c.get());
        conns_.clear();
        if (listen_fd_ >= 0) ::close(listen_fd_);
        ::close(wake_pipe_[0]);
        ::close(wake_pipe_[1]);
        listen_fd_ = -1;
        ::unlink(path_.c_str());
    }

  private:
    // ---------------- nghttp2 callbacks ----------------

    static int on_begin_headers(nghttp2_session *, const nghttp2_frame *frame,
                                void *user) {
        auto *conn = static_cast<Conn *>(user);
        if (frame->hd.type == NGHTTP2_FRAME_HEADERS) {
            auto st = std::make_unique<Stream>();
            st->conn = conn;
            conn->streams[frame->hd.stream_id] = std::move(st);
        }
        return 0;
    }

    static int on_header(nghttp2_session *, const nghttp2_frame *frame,
                         const uint8_t *name, size_t namelen,
                         const uint8_t *value, size_t valuelen, uint8_t,
                         void *user) {
        auto *conn = static_cast<Conn *>(user);
        auto it = conn->streams.find(frame->hd.stream_id);
        if (it == conn->streams.end()) return 0;
        if (namelen == 5 && memcmp(name, ":path", 5) == 0)
            it->second->path.assign((const char *)value, valuelen);
        return 0;
    }

    static int on_data_chunk(nghttp2_session *, uint8_t, int32_t stream_id,
                             const uint8_t *data, size_t len, void *user) {
        auto *conn = static_cast<Conn *>(user);
        auto it = conn->streams.find(stream_id);
        if (it != conn->streams.end())
            it->second->req_body.append((const char *)data, len);
        return 0;
    }

    static int on_frame_recv(nghttp2_session *, const nghttp2_frame *frame,
                             void *user) {
        auto *conn = static_cast<Conn *>(user);
        if ((frame->hd.type == NGHTTP2_FRAME_HEADERS ||
             frame->hd.type == NGHTTP2_FRAME_DATA) &&
            (frame->hd.flags & NGHTTP2_FLAG_END_STREAM)) {
            auto it = conn->streams.find(frame->hd.stream_id);
            if (it != conn->streams.end())
                conn->srv->dispatch(conn, frame->hd.stream_id,
                                    it->second.get());
        }
        return 0;
    }

    static int on_stream_close(nghttp2_session *, int32_t stream_id, uint32_t,
                               void *user) {
        auto *conn = static_cast<Conn *>(user);
        conn->streams.erase(stream_id);
        return 0;
    }

    static ssize_t data_read(nghttp2_session *, int32_t stream_id, uint8_t *buf,
                             size_t length, uint32_t *data_flags,
                             nghttp2_data_source *source, void *user) {
        auto *conn = static_cast<Conn *>(user);
        auto *st = static_cast<Stream *>(source->ptr);
        auto &ng = NgHttp2::get();
        size_t avail;
        {
            std::lock_guard<std::mutex> g(conn->srv->mu_);
            avail = st->out.size() - st->out_off;
            if (avail == 0 && st->is_listwatch) return NGHTTP2_ERR_DEFERRED;
            size_t n = std::min(avail, length);
            memcpy(buf, st->out.data() + st->out_off, n);
            st->out_off += n;
            avail -= n;
            if (st->is_listwatch) {
                if (st->out_off == st->out.size()) {
                    st->out.clear();
                    st->out_off = 0;
                }
                // server-streaming: never EOF until shutdown
                return (ssize_t)n;
            }
            if (avail == 0) {
                *data_flags |= NGHTTP2_DATA_FLAG_EOF | NGHTTP2_DATA_FLAG_NO_END_STREAM;
                if (!st->trailer_sent) {
                    st->trailer_sent = true;
                    nghttp2_nv tr[2];
                    static const char kStatus[] = "grpc-status";
                    static const char kMsg[] = "grpc-message";
                    tr[0] = {(uint8_t *)kStatus, (uint8_t *)st->grpc_status.data(),
                             sizeof(kStatus) - 1, st->grpc_status.size(),
                             NGHTTP2_NV_FLAG_NONE};
                    size_t ntr = 1;
                    if (!st->grpc_message.empty()) {
                        tr[1] = {(uint8_t *)kMsg,
                                 (uint8_t *)st->grpc_message.data(),
                                 sizeof(kMsg) - 1, st->grpc_message.size(),
                                 NGHTTP2_NV_FLAG_NONE};
                        ntr = 2;
                    }
                    ng.submit_trailer(conn->session, stream_id, tr, ntr);
                }
            }
            return (ssize_t)n;
        }
    }

    // ---------------- request dispatch ----------------

    void dispatch(Conn *conn, int32_t stream_id, Stream *st) {
        // Validate the gRPC length-prefixed message framing before looking
        // at the path.  A compressed-flag byte other than 0 means the
        // client negotiated a message codec we do not implement
        // (grpc-go only sets it after a grpc-encoding handshake) →
        // UNIMPLEMENTED(12), matching grpc-go's own unsupported-codec
        // status.  A body shorter than the declared length (truncated
        // frame) or a stray partial prefix is a malformed request →
        // INTERNAL(13).  Treating either as an empty request would turn
        // garbage into a bogus success (e.g. an Allocate response with
        // only /dev/kfd).
        const uint8_t *msg = nullptr;
        size_t msg_len = 0;
        if (!st->req_body.empty()) {
            if (st->req_body.size() < 5)  // INTERNAL: truncated frame prefix
                return submit_error(conn, stream_id, st, "13",
                                    "malformed grpc frame: short prefix");
            uint8_t compressed = (uint8_t)st->req_body[0];
            uint32_t len;
            memcpy(&len, st->req_body.data() + 1, 4);
            len = ntohl(len);
            if (compressed != 0)  // UNIMPLEMENTED: compression
                return submit_error(conn, stream_id, st, "12",
                                    "grpc message compression not supported");
            if (st->req_body.size() < (size_t)5 + len)  // INTERNAL
                return submit_error(conn, stream_id, st, "13",
                                    "malformed grpc frame: truncated body");
            msg = (const uint8_t *)st->req_body.data() + 5;
            msg_len = len;
        }

        const std::string &p = st->path;
        std::string resp(kGrpcPrefix, '\0');  // framed in submit_unary
        if (p == "/v1beta1.DevicePlugin/GetDevicePluginOptions") {
            n_options_.fetch_add(1, std::memory_order_relaxed);
            std::lock_guard<std::mutex> g(mu_);
            resp += options_;
        } else if (p == "/v1beta1.DevicePlugin/PreStartContainer") {
            n_prestart_.fetch_add(1, std::memory_order_relaxed);
            std::string bad;
            if (!handle_prestart(msg, msg_len, bad))  // FAILED_PRECONDITION
                return submit_error(
                    conn, stream_id, st, "9",
                    "device " + bad + " failed the pre-start probe");
        } else if (p == "/v1beta1.DevicePlugin/Allocate") {
            n_allocate_.fetch_add(1, std::memory_order_relaxed);
            auto t0 = std::chrono::steady_clock::now();
            handle_allocate(msg, msg_len, resp);
            allocate_ns_.fetch_add(
                (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                    std::chrono::steady_clock::now() - t0).count(),
                std::memory_order_relaxed);
        } else if (p == "/v1beta1.DevicePlugin/GetPreferredAllocation") {
            n_preferred_.fetch_add(1, std::memory_order_relaxed);
            auto t0 = std::chrono::steady_clock::now();
            std::string err;
            bool ok = handle_preferred(msg, msg_len, resp, err);
            preferred_ns_.fetch_add(
                (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                    std::chrono::steady_clock::now() - t0).count(),
                std::memory_order_relaxed);
            if (!ok)  // INVALID_ARGUMENT
                return submit_error(conn, stream_id, st, "3", err);
        } else if (p == "/v1beta1.DevicePlugin/ListAndWatch") {
            n_listwatch_.fetch_add(1, std::memory_order_relaxed);
            st->is_listwatch = true;
            {
                std::lock_guard<std::mutex> g(mu_);
                st->out = grpc_frame(list_bytes_);
                st->out_off = 0;
            }
            submit_headers_common(conn, stream_id, st);
            return;
        } else {
            n_unknown_.fetch_add(1, std::memory_order_relaxed);
            return submit_error(conn, stream_id, st, "12", "");  // UNIMPLEMENTED
        }
        submit_unary(conn, stream_id, st, std::move(resp));
    }

    // trailers-only style failure: no message body, status in the trailer
    void submit_error(Conn *conn, int32_t stream_id, Stream *st,
                      const char *status, const std::string &message) {
        st->grpc_status = status;
        st->grpc_message = message;
        submit_unary(conn, stream_id, st, std::string());
    }

    void submit_headers_common(Conn *conn, int32_t stream_id, Stream *st) {
        auto &ng = NgHttp2::get();
        static const char kS[] = ":status", k200[] = "200";
        static const char kCT[] = "content-type", kGrpc[] = "application/grpc";
        nghttp2_nv hdrs[2] = {
            {(uint8_t *)kS, (uint8_t *)k200, sizeof(kS) - 1, sizeof(k200) - 1,
             NGHTTP2_NV_FLAG_NONE},
            {(uint8_t *)kCT, (uint8_t *)kGrpc, sizeof(kCT) - 1,
             sizeof(kGrpc) - 1, NGHTTP2_NV_FLAG_NONE},
        };
        nghttp2_data_provider prov;
        prov.source.ptr = st;
        prov.read_callback = data_read;
        ng.submit_response(conn->session, stream_id, hdrs, 2, &prov);
    }

    // `framed` is empty (no body) or kGrpcPrefix placeholder bytes followed
    // by the message
    void submit_unary(Conn *conn, int32_t stream_id, Stream *st,
                      std::string &&framed) {
        if (!framed.empty()) grpc_frame_in_place(framed);
        {
            std::lock_guard<std::mutex> g(mu_);
            st->out = std::move(framed);
            st->out_off = 0;
        }
        submit_headers_common(conn, stream_id, st);
    }

    // true = every requested device opens; on failure `bad` names it
    bool handle_prestart(const uint8_t *p, size_t msg_len, std::string &bad) {
        std::unordered_map<std::string, std::string> paths;
        {
            std::lock_guard<std::mutex> g(mu_);
            if (prestart_paths_.empty()) return true;  // probe disabled
            paths = prestart_paths_;
        }
        bool ok = true;
        for_each_field(p, p + msg_len, [&](int field, int wt,
                                           const uint8_t *data,
                                           uint64_t len) {
            if (!ok || field != 1 || wt != 2) return;
            std::string id((const char *)data, len);
            auto it = paths.find(id);
            if (it == paths.end()) return;
            int fd = ::open(it->second.c_str(), O_RDWR | O_CLOEXEC);
            if (fd < 0) {
                ok = false;
                bad = id;
            } else {
                ::close(fd);
            }
        });
        return ok;
    }

    // appends the AllocateResponse to resp
    void handle_allocate(const uint8_t *p, size_t msg_len, std::string &resp) {
        std::lock_guard<std::mutex> g(mu_);
        std::string &car = car_;
        for_each_field(p, p + msg_len, [&](int field, int wt,
                                           const uint8_t *data,
                                           uint64_t len) {
            if (field != 1 || wt != 2) return;
            // one ContainerAllocateRequest
            car = kfd_spec_;
            for_each_field(data, data + len, [&](int f2, int wt2,
                                                 const uint8_t *d2,
                                                 uint64_t l2) {
                if (f2 != 1 || wt2 != 2) return;
                std::string id((const char *)d2, l2);
                auto it = dev_specs_.find(id);
                if (it != dev_specs_.end()) car += it->second;
            });
            put_len_delim(resp, 1, car);
        });
    }

    // appends the PreferredAllocationResponse to resp; the id lists, the
    // response fragment and the search's scratch are members, reused from
    // request to request (only this thread runs handlers, under mu_)
    bool handle_preferred(const uint8_t *p, size_t msg_len, std::string &resp,
                          std::string &err) {
        std::lock_guard<std::mutex> g(mu_);
        bool ok = true;
        std::vector<std::string> &available = pref_available_,
                                 &required = pref_required_,
                                 &chosen = pref_chosen_;
        std::string &car = car_;
        for_each_field(p, p + msg_len, [&](int field, int wt,
                                           const uint8_t *data,
                                           uint64_t len) {
            if (!ok || field != 1 || wt != 2) return;
            available.clear();
            required.clear();
            chosen.clear();
            int size = 0;
            for_each_field(data, data + len, [&](int f2, int wt2,
                                                 const uint8_t *d2,
                                                 uint64_t l2) {
                if (f2 == 1 && wt2 == 2)
                    available.emplace_back((const char *)d2, l2);
                else if (f2 == 2 && wt2 == 2)
                    required.emplace_back((const char *)d2, l2);
                else if (f2 == 3 && wt2 == 0)
                    size = (int)l2;
            });
            if (!preferred_alloc(alloc_, scratch_, available, required, size,
                                 chosen, err)) {
                ok = false;
                return;
            }
            car.clear();
            for (auto &id : chosen) put_len_delim(car, 1, id);
            put_len_delim(resp, 1, car);
        });
        return ok;
    }

    // ---------------- event loop ----------------

    void wake() {
        char c = 1;
        ssize_t rc = ::write(wake_pipe_[1], &c, 1);
        (void)rc;
    }

    // Connection cap: the kubelet needs 1-2 connections; a runaway local
    // client must not exhaust the daemon's fds (the socket dir is
    // root-only, so this is belt-and-braces, not a security boundary).
    static constexpr size_t kMaxConns = 256;

    void accept_conn() {
        for (;;) {
            int fd = ::accept4(listen_fd_, nullptr, nullptr, SOCK_NONBLOCK);
            if (fd < 0) return;
            if (conns_.size() >= kMaxConns) {
                ::close(fd);  // refuse; peer sees ECONNRESET and retries
                continue;
            }
            auto &ng = NgHttp2::get();
            nghttp2_session_callbacks *cbs;
            ng.session_callbacks_new(&cbs);
            ng.set_on_begin_headers(cbs, on_begin_headers);
            ng.set_on_header(cbs, on_header);
            ng.set_on_data_chunk_recv(cbs, on_data_chunk);
            ng.set_on_frame_recv(cbs, on_frame_recv);
            ng.set_on_stream_close(cbs, on_stream_close);
            auto conn = std::make_unique<Conn>();
            conn->fd = fd;
            conn->srv = this;
            ng.session_server_new(&conn->session, cbs, conn.get());
            ng.session_callbacks_del(cbs);
            nghttp2_settings_entry st[1] = {
                {NGHTTP2_SETTINGS_MAX_CONCURRENT_STREAMS, 128}};
            ng.submit_settings(conn->session, NGHTTP2_FLAG_NONE, st, 1);
            n_conns_.fetch_add(1, std::memory_order_relaxed);
            conns_.push_back(std::move(conn));
        }
    }

    void destroy_conn(Conn *c) {
        auto &ng = NgHttp2::get();
        if (c->session) ng.session_del(c->session);
        if (c->fd >= 0) ::close(c->fd);
        c->session = nullptr;
        c->fd = -1;
        c->dead = true;
    }

    // How much is gathered before a write: about one read buffer.  A
    // large ListAndWatch response or a burst of pipelined responses goes
    // out in pieces of this size instead of growing the buffer.
    static constexpr size_t kGatherLimit = 65536;

    // Sends what the session has ready: everything session_mem_send()
    // hands back (one frame per call) is gathered into the connection's
    // buffer and goes out with one write(), so a unary response (HEADERS,
    // DATA, trailer HEADERS) is one syscall.  When the socket takes less
    // than it was offered the unsent tail stays, in order, behind an
    // offset, and POLLOUT drives the rest.  Returns false when the
    // connection died.
    bool flush_conn(Conn *c) {
        auto &ng = NgHttp2::get();
        for (;;) {
            if (!c->want_out()) {
                c->wbuf.clear();
                c->woff = 0;
            } else if (c->woff >= kGatherLimit) {
                // drop the sent prefix once it outweighs the tail, so a
                // long back-pressured stream does not keep what it sent
                c->wbuf.erase(0, c->woff);
                c->woff = 0;
            }
            while (c->wbuf.size() - c->woff < kGatherLimit) {
                const uint8_t *data = nullptr;
                ssize_t len = ng.session_mem_send(c->session, &data);
                if (len < 0) return false;
                if (len == 0) break;
                c->wbuf.append((const char *)data, (size_t)len);
            }
            if (!c->want_out()) return true;
            size_t want = c->wbuf.size() - c->woff;
            ssize_t n = ::write(c->fd, c->wbuf.data() + c->woff, want);
            n_writes_.fetch_add(1, std::memory_order_relaxed);
            if (n < 0) {
                if (errno == EINTR) continue;
                if (errno == EAGAIN || errno == EWOULDBLOCK) {
                    n_would_block_.fetch_add(1, std::memory_order_relaxed);
                    return true;
                }
                return false;
            }
            c->woff += (size_t)n;
            if ((size_t)n < want) {  // the socket is full: wait for POLLOUT
                n_would_block_.fetch_add(1, std::memory_order_relaxed);
                return true;
            }
        }
    }

    void run_loop() {
        auto &ng = NgHttp2::get();
        std::vector<pollfd> pfds;
        uint8_t buf[65536];
        while (running_.load()) {
            pfds.clear();
            pfds.push_back({listen_fd_, POLLIN, 0});
            pfds.push_back({wake_pipe_[0], POLLIN, 0});
            for (auto &c : conns_) {
                short ev = POLLIN;
                if (c->want_out() || ng.session_want_write(c->session))
                    ev |= POLLOUT;
                pfds.push_back({c->fd, ev, 0});
            }
            int rc = ::poll(pfds.data(), pfds.size(), 500);
            if (rc < 0 && errno != EINTR) break;
            if (!running_.load()) break;

            if (pfds[1].revents & POLLIN) {
                char tmp[64];
                while (::read(wake_pipe_[0], tmp, sizeof(tmp)) > 0) {
                }
                bool do_push;
                std::string bytes;
                {
                    std::lock_guard<std::mutex> g(mu_);
                    do_push = pending_push_;
                    pending_push_ = false;
                    bytes = list_bytes_;
                }
                if (do_push) {
                    n_pushes_.fetch_add(1, std::memory_order_relaxed);
                    std::string framed = grpc_frame(bytes);
                    for (auto &c : conns_) {
                        for (auto &skv : c->streams) {
                            Stream *st = skv.second.get();
                            if (!st->is_listwatch) continue;
                            {
                                std::lock_guard<std::mutex> g(mu_);
                                st->out += framed;
                            }
                            ng.session_resume_data(c->session, skv.first);
                        }
                    }
                }
            }

            if (pfds[0].revents & POLLIN) accept_conn();

            size_t pi = 2;
            for (auto &c : conns_) {
                short rev = pi < pfds.size() ? pfds[pi].revents : 0;
                ++pi;
                if (c->dead) continue;
                if (rev & (POLLERR | POLLHUP)) {
                    destroy_conn(c.get());
                    continue;
                }
                if (rev & POLLIN) {
                    // poll is level-triggered: after a read that did not
                    // fill the buffer, whatever arrives later is reported
                    // by the next poll, so there is no read just to see
                    // EAGAIN
                    for (;;) {
                        ssize_t n = ::read(c->fd, buf, sizeof(buf));
                        n_reads_.fetch_add(1, std::memory_order_relaxed);
                        if (n > 0) {
                            if (ng.session_mem_recv(c->session, buf,
                                                    (size_t)n) < 0) {
                                destroy_conn(c.get());
                                break;
                            }
                            if ((size_t)n < sizeof(buf)) break;
                        } else if (n == 0) {
                            destroy_conn(c.get());
                            break;
                        } else {
                            if (errno != EAGAIN && errno != EWOULDBLOCK)
                                destroy_conn(c.get());
                            break;
                        }
                    }
                }
                if (!c->dead && !flush_conn(c.get()))
                    destroy_conn(c.get());
            }
            conns_.erase(std::remove_if(conns_.begin(), conns_.end(),
                                        [](auto &c) { return c->dead; }),
                         conns_.end());
        }
    }

    std::string path_;
    int listen_fd_ = -1;
    int wake_pipe_[2] = {-1, -1};
    std::thread loop_;
    std::atomic<bool> running_{false};
    std::vector<std::unique_ptr<Conn>> conns_;

    std::atomic<uint64_t> allocate_ns_{0}, preferred_ns_{0};
    std::atomic<uint64_t> n_allocate_{0}, n_preferred_{0}, n_listwatch_{0},
        n_options_{0}, n_prestart_{0}, n_unknown_{0}, n_pushes_{0},
        n_conns_{0}, n_writes_{0}, n_reads_{0}, n_would_block_{0};

    std::mutex mu_;
    std::string options_, kfd_spec_, list_bytes_;
    std::unordered_map<std::string, std::string> dev_specs_;
    std::unordered_map<std::string, std::string> prestart_paths_;
    AllocState alloc_;
    // request-path buffers, reused; touched only under mu_
    prefalloc::Scratch scratch_;
    std::vector<std::string> pref_available_, pref_required_, pref_chosen_;
    std::string car_;
    bool pending_push_ = false;
};

}  // namespace

PYBIND11_MODULE(_fastserver, m) {
    m.doc() = "native DevicePlugin v1beta1 gRPC server (nghttp2 over UDS)";
    py::class_<Server>(m, "Server")
        .def(py::init<std::string>())
        .def("set_options_response", &Server::set_options_response)
        .def("set_kfd_spec", &Server::set_kfd_spec)
        .def("set_device_specs", &Server::set_device_specs)
        .def("set_list_response", &Server::set_list_response)
        .def("push_list_update", &Server::push_list_update)
        .def("set_allocator_state", &Server::set_allocator_state)
        .def("stats", &Server::stats)
        .def("set_prestart_paths", &Server::set_prestart_paths)
        .def("start", &Server::start,
             py::call_guard<py::gil_scoped_release>())
        .def("stop", &Server::stop, py::call_guard<py::gil_scoped_release>());
}
