// HIP evaluator runtime: uploads a batch of B garbled models (same circuit,
// independent garblings) into an HBM arena and evaluates them together, one
// kernel launch per gadget phase over (GC x residue x element). All launches
// go to one stream (no per-layer device synchronisation, unlike the
// reference's cudaDeviceSynchronize after every layer), so the whole forward
// can be captured into a hipGraph.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <atomic>
#include <cstring>
#include <tuple>
#include <chrono>
#include <map>
#include <mutex>
#include <functional>
#include <thread>

#include "../layers.h"
#include "host_util.h"
#include "launch.h"
#include "fetch.h"
#include "gpu_garbler.h"

#include <rocprofiler-sdk-roctx/roctx.h>

namespace py = pybind11;

namespace dash {
using namespace dev;

using namespace hostutil;

// ---------------------------------------------------------------------------
// Garbler side of the same-node device transport: another process's evaluator table arenas opened through their
// IPC handles (HipEvaluator::ipc_export), handed to the GPU garbler as slot sinks. The garbler's kernels write
// the tables straight into the evaluator's HBM (its own device, or a peer over xGMI); only the skeleton of each
// model (constants, shapes) then travels over the channel.
class IpcTables {
   public:
    IpcTables(int device, const std::vector<std::tuple<size_t, std::string, size_t, std::string>>& handles, int B)
        : dev_(device), B_(B), alive_(std::make_shared<std::atomic<bool>>(true)) {
        DASH_CHECK(B >= 1, "IpcTables: batch must be >= 1");
        bind_device(dev_, nullptr, "IpcTables");
        for (const auto& h : handles) {
            const std::string& hb = std::get<3>(h);
            DASH_CHECK(hb.size() == sizeof(hipIpcMemHandle_t), "IpcTables: bad IPC handle size");
            hipIpcMemHandle_t mh;
            std::memcpy(&mh, hb.data(), sizeof(mh));
            void* p = nullptr;
            HIPCHECK(hipIpcOpenMemHandle(&p, mh, hipIpcMemLazyEnablePeerAccess));
            opened_.push_back(p);
            map_[{std::get<0>(h), std::get<1>(h)}] = {static_cast<uint8_t*>(p), std::get<2>(h)};
        }
    }
    ~IpcTables() {
        alive_->store(false);
        (void)hipSetDevice(dev_);
        for (void* p : opened_) (void)hipIpcCloseMemHandle(p);
        (void)hipGetLastError();  // teardown errors are ignored: do not leave them for a later HIPCHECK
    }
    int tables() const { return static_cast<int>(map_.size()); }
    std::shared_ptr<TableSink> sink(int b) const {
        DASH_CHECK(b >= 0 && b < B_, "IpcTables: batch slot out of range");
        auto map = map_;
        const int dev = dev_;
        auto alive = alive_;
        auto s = std::make_shared<TableSink>();
        s->dest = [map, b, dev, alive](size_t layer, const std::string& name, size_t nbytes) -> std::shared_ptr<Array::Device> {
            auto it = map.find({layer, name});
            if (it == map.end() || it->second.second != nbytes) return nullptr;
            auto d = std::make_shared<Array::Device>();
            d->p = std::shared_ptr<void>(it->second.first + nbytes * b, [](void*) {});  // the evaluator owns it
            d->device = dev;
            d->external = true;
            d->fetch = [dev, alive](void* h, const void* dv, size_t n) {
                if (!alive->load())
                    throw std::runtime_error("dash: tables live in a closed IPC mapping of the evaluator's slots");
                HIPCHECK(hipSetDevice(dev));
                HIPCHECK(hipMemcpy(h, dv, n, hipMemcpyDeviceToHost));
            };
            return d;
        };
        return s;
    }

   private:
    int dev_, B_;
    std::shared_ptr<std::atomic<bool>> alive_;
    std::vector<void*> opened_;
    std::map<std::pair<size_t, std::string>, std::pair<uint8_t*, size_t>> map_;
};

// ---------------------------------------------------------------------------
class HipEvaluator {
   public:
    HipEvaluator(std::shared_ptr<GarbledModel> tmpl, int B, int device, bool use_mfma, bool stream_tables = false)
        : tmpl_(std::move(tmpl)), mfma_(use_mfma), stream_(stream_tables) {
        DASH_CHECK(tmpl_ && B >= 1, "HipEvaluator needs a template model and B >= 1");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw std::runtime_error("dash: no HIP device available for HipEvaluator");
        dev_ = device;
        HIPCHECK(hipSetDevice(dev_));
        B_ = B;
        crt_ = tmpl_->h.crt;
        k_ = static_cast<int>(crt_.size());
        for (int p : crt_)
            DASH_CHECK(p <= kActMaxModulus, "HIP evaluator: CRT modulus " + std::to_string(p) +
                                                " > 255 (activations are stored as bytes); use the host evaluator");
        DASH_CHECK(k_ <= kMaxRes, "too many CRT residues for the GPU path");
        loaded_.assign(B_, 0);
        build();
        // Keep only what load() checks: holding the template model would pin
        // its garbled tables (10 GB per MiniONN GC, device-resident when the
        // GPU garbler made them) for the evaluator's lifetime.
        tmpl_h_ = tmpl_->h;
        tmpl_nlayers_ = tmpl_->layers.size();
        tmpl_.reset();
    }
    // Upload garbled model `m` (same circuit as the template) into batch slot b.
    void load(int b, const GarbledModel& m) {
        DASH_CHECK(b >= 0 && b < B_, "batch slot out of range");
        // one load at a time: the per-GC constants go through ONE pinned staging block, device block and load
        // stream shared by all slots (the serving engine's refill workers load different slots of one evaluator
        // concurrently; unserialized, one slot's constants could land in another's)
        std::lock_guard<std::mutex> load_guard(load_mu_);
        DASH_CHECK(m.h.crt == tmpl_h_.crt && m.h.mrs == tmpl_h_.mrs && m.layers.size() == tmpl_nlayers_ &&
                       m.h.in_dims == tmpl_h_.in_dims && m.h.hardened == tmpl_h_.hardened,
                   "model does not garble the evaluator's circuit (or uses another encoding)");
        bind_device(dev_, load_st_, "HipEvaluator.load");
        if (!load_st_) HIPCHECK(hipStreamCreateWithFlags(&load_st_, hipStreamNonBlocking));
        // per-GC small constants (bias labels, zero / shift labels, ...): filled into one pinned staging block,
        // one H2D copy and one scatter kernel to their slot-b destinations, instead of ~100 small copies
        if (!small_.empty()) {
            for (const auto& c : small_) c.fill(m, small_h_ + c.off);
            HIPCHECK(hipMemcpyAsync(small_d_, small_h_, small_bytes_, hipMemcpyHostToDevice, load_st_));
            launch_scatter(small_desc_, static_cast<int>(small_.size()), small_d_, b, load_st_);
        }
        // tables (a GC garbled into this slot through sink() needs none of these copies)
        for (auto& f : loaders_) f(b, m);
        // evaluation and garbling streams are non-blocking: this waits for this load only
        HIPCHECK(hipStreamSynchronize(load_st_));
        loaded_[b] = 1;
    }
    // Zero-copy offline phase (GarbleOptions::sink): slot b's table arenas as GPU-garbler destinations.
    // A model garbled with this sink already has its tables in slot b, and load(b, m) skips their copies.
    std::shared_ptr<TableSink> sink(int b) const {
        DASH_CHECK(b >= 0 && b < B_, "batch slot out of range");
        auto arena = arena_;
        const int dev = dev_;
        auto alive = alive_;
        auto s = std::make_shared<TableSink>();
        s->dest = [arena, b, dev, alive](size_t layer, const std::string& name, size_t nbytes) -> std::shared_ptr<Array::Device> {
            auto it = arena.find({layer, name});
            if (it == arena.end() || it->second.second != nbytes) return nullptr;
            auto d = std::make_shared<Array::Device>();
            d->p = std::shared_ptr<void>(it->second.first + nbytes * b, [](void*) {});  // the evaluator owns it
            d->device = dev;
            d->external = true;
            // the arena belongs to the evaluator: a model that outlives it must not read freed HBM
            d->fetch = [dev, alive](void* h, const void* dv, size_t n) {
                if (!alive->load())
                    throw std::runtime_error("dash: garbled tables live in a destroyed HipEvaluator's slot (sink); "
                                             "the model is no longer readable");
                HIPCHECK(hipSetDevice(dev));
                HIPCHECK(hipMemcpy(h, dv, n, hipMemcpyDeviceToHost));
            };
            return d;
        };
        return s;
    }
    // Same-node device transport (net/protocol.py, transport "ipc"): an IPC handle per table arena, so a
    // garbler process can garble straight into this evaluator's slots (IpcTables). Entries: (layer, table,
    // bytes per slot, handle bytes).
    std::vector<std::tuple<size_t, std::string, size_t, std::string>> ipc_export() const {
        bind_device(dev_, nullptr, "HipEvaluator.ipc_export");
        DASH_CHECK(!stream_, "ipc export needs HBM-resident tables (stream_tables=False)");
        std::vector<std::tuple<size_t, std::string, size_t, std::string>> out;
        for (const auto& kv : arena_) {
            hipIpcMemHandle_t h;
            HIPCHECK(hipIpcGetMemHandle(&h, kv.second.first));
            out.emplace_back(kv.first.first, kv.first.second, kv.second.second,
                             std::string(reinterpret_cast<const char*>(&h), sizeof(h)));
        }
        return out;
    }
    ~HipEvaluator() {
        alive_->store(false);  // orphans every sink-backed model array (fetch raises instead of reading freed HBM)
        if (copy_st_) (void)hipStreamSynchronize(copy_st_);
        for (auto e : ready_) (void)hipEventDestroy(e);
        for (auto e : done_) (void)hipEventDestroy(e);
        if (run_end_) (void)hipEventDestroy(run_end_);
        if (copy_st_) (void)hipStreamDestroy(copy_st_);
        if (load_st_) (void)hipStreamDestroy(load_st_);
        if (gexec_) (void)hipGraphExecDestroy(gexec_);
        for (void* p : allocs_) (void)hipFree(p);
        for (void* p : host_allocs_) (void)hipHostFree(p);
        (void)hipGetLastError();  // teardown errors are ignored: do not leave them for a later HIPCHECK
    }

    int batch() const { return B_; }
    bool streams_tables() const { return stream_; }
    size_t device_bytes() const { return dev_bytes_; }
    size_t table_bytes() const { return table_bytes_; }

    void set_inputs(const std::vector<CrtLabels>& in, hipStream_t st) {
        DASH_CHECK(static_cast<int>(in.size()) == B_, "need one input per garbled model in the batch");
        for (int j = 0; j < k_; ++j) {
            const int n = nr_comps(crt_[j]);
            int16_t* stg = in_stage_[j];
            for (int b = 0; b < B_; ++b) {
                const Labels& L = in[b][j];
                DASH_CHECK(L.p == crt_[j] && L.N == N0_, "input label shape mismatch");
                for (i64 e = 0; e < N0_; ++e)
                    for (int c = 0; c < n; ++c) stg[(static_cast<i64>(b) * n + c) * N0_ + e] = L.c[e * n + c];
            }
        }
        upload_inputs(st);
    }

    // pinned staging slots for GC b (one component-major block per residue)
    std::vector<int16_t*> input_slot(int b) const {
        DASH_CHECK(b >= 0 && b < B_, "batch slot out of range");
        std::vector<int16_t*> v;
        for (int j = 0; j < k_; ++j) v.push_back(in_stage_[j] + static_cast<i64>(b) * nr_comps(crt_[j]) * N0_);
        return v;
    }
    i64 input_size() const { return N0_; }
    int device() const { return dev_; }
    const std::vector<int>& crt() const { return crt_; }
    // slot b's device input activations of residue j, [n_j][N0] bytes: the target of the garbler's device encoder
    act_t* input_act(int b, int j) const {
        DASH_CHECK(b >= 0 && b < B_ && j >= 0 && j < k_, "input slot out of range");
        return bufs_[0].p[j] + static_cast<i64>(b) * nr_comps(crt_[j]) * N0_;
    }
    // compressed staging (online message #1 in wire form): [B][k][N0] u128
    u128* input_slot_compressed(int b) {
        DASH_CHECK(b >= 0 && b < B_, "batch slot out of range");
        if (!in_comp_stage_) {
            bind_device(dev_, nullptr, "HipEvaluator.input_slot_compressed");
            const size_t bytes = sizeof(u128) * B_ * k_ * N0_;
            HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&in_comp_stage_), bytes));
            host_allocs_.push_back(in_comp_stage_);
            HIPCHECK(hipMalloc(reinterpret_cast<void**>(&in_comp_dev_), bytes));
            allocs_.push_back(in_comp_dev_);
            dev_bytes_ += bytes;
        }
        return in_comp_stage_ + static_cast<i64>(b) * k_ * N0_;
    }
    void upload_inputs_compressed(hipStream_t st) {
        bind_device(dev_, st, "HipEvaluator.upload_inputs_compressed");
        DASH_CHECK(in_comp_stage_ != nullptr, "no compressed inputs staged");
        HIPCHECK(hipMemcpyAsync(in_comp_dev_, in_comp_stage_, sizeof(u128) * B_ * k_ * N0_, hipMemcpyHostToDevice, st));
        launch_unpack(in_comp_dev_, k_, bufs_[0], crt_info(crt_), mc_, N0_, B_, st);
    }
    // output labels of slot b, compressed on the host: [k][Nout]
    std::vector<u128> outputs_compressed(int b) const {
        std::vector<u128> r(static_cast<size_t>(k_) * Nout_);
        for (int j = 0; j < k_; ++j) {
            const ModInfo& mi = mod_info(out_mod_[j]);
            comp_t buf[128];
            for (i64 e = 0; e < Nout_; ++e) {
                for (int c = 0; c < mi.n; ++c) buf[c] = out_stage_[j][(static_cast<i64>(b) * mi.n + c) * Nout_ + e];
                r[static_cast<size_t>(j) * Nout_ + e] = compress(buf, mi);
            }
        }
        return r;
    }
    // every residue's output labels -> out_stage_: one k_fetch_res launch into the mapped pinned buffers for small
    // outputs (one launch instead of k copy-engine transfers), copies otherwise or with DASH_FETCH_KERNEL=0 (A/B)
    void stage_outputs(hipStream_t st) {
        static const bool kern = [] {
            const char* e = std::getenv("DASH_FETCH_KERNEL");
            return !(e && e[0] == '0');
        }();
        FetchRes f{};
        f.k = k_;
        int64_t total = 0;
        for (int j = 0; j < k_; ++j) {
            f.in[j] = final_.p[j];
            f.out[j] = out_stage_dev_[j];
            f.bytes[j] = static_cast<int64_t>(sizeof(act_t)) * B_ * nr_comps(out_mod_[j]) * Nout_;
            total += f.bytes[j];
        }
        if (kern && total <= (4 << 20) && out_stage_mapped_) {
            launch_fetch_res(f, st);
            HIPCHECK(hipGetLastError());
        } else {
            for (int j = 0; j < k_; ++j)
                HIPCHECK(hipMemcpyAsync(out_stage_[j], final_.p[j], f.bytes[j], hipMemcpyDeviceToHost, st));
        }
        HIPCHECK(hipStreamSynchronize(st));
    }
    void fetch_outputs(hipStream_t st) {
        bind_device(dev_, st, "HipEvaluator.fetch_outputs");
        stage_outputs(st);
    }
    int crt_size() const { return k_; }
    i64 output_size() const { return Nout_; }
    // int16 host staging (the host label format) -> device int16 scratch -> byte activations
    void upload_inputs(hipStream_t st) {
        bind_device(dev_, st, "HipEvaluator.upload_inputs");
        for (int j = 0; j < k_; ++j) {
            const i64 count = static_cast<i64>(B_) * nr_comps(crt_[j]) * N0_;
            if (!in16_dev_[j]) in16_dev_[j] = dalloc<int16_t>(static_cast<size_t>(count));
            HIPCHECK(hipMemcpyAsync(in16_dev_[j], in_stage_[j], sizeof(int16_t) * count, hipMemcpyHostToDevice, st));
            launch_narrow(in16_dev_[j], bufs_[0].p[j], count, st);
        }
    }

    // The op list is static (all device pointers fixed at build time), so
    // after one eager run (lazy one-time allocations) it is captured into a
    // hipGraph and replayed: one launch per evaluation instead of ~200.
    void run(hipStream_t st) {
        bind_device(dev_, st, "HipEvaluator.run");
        for (int b = 0; b < B_; ++b) DASH_CHECK(loaded_[b], "batch slot " + std::to_string(b) + " has no garbled model loaded");
        if (profile_ || !use_graph_ || runs_ == 0 || st == nullptr) {
            // roctx ranges per op (layer / gadget phase) for rocprofv3 --marker-trace (DASH_ROCTX=1)
            static const bool markers = [] {
                const char* e = std::getenv("DASH_ROCTX");
                return e && e[0] == '1';
            }();
            for (size_t i = 0; i < ops_.size(); ++i) {
                if (profile_) HIPCHECK(hipEventRecord(ev_[i], st));
                if (markers) roctxRangePushA(op_names_[i].c_str());
                ops_[i](st);
                if (markers) roctxRangePop();
            }
            if (profile_) HIPCHECK(hipEventRecord(ev_.back(), st));
            HIPCHECK(hipGetLastError());
            ++runs_;
            return;
        }
        if (!gexec_ || gstream_ != st) {
            if (gexec_) HIPCHECK(hipGraphExecDestroy(gexec_));
            gexec_ = nullptr;
            hipGraph_t graph = nullptr;
            HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
            for (auto& op : ops_) op(st);
            HIPCHECK(hipStreamEndCapture(st, &graph));
            HIPCHECK(hipGraphInstantiate(&gexec_, graph, nullptr, nullptr, 0));
            HIPCHECK(hipGraphDestroy(graph));
            gstream_ = st;
        }
        HIPCHECK(hipGraphLaunch(gexec_, st));
        ++runs_;
    }
    void set_graph(bool on) { use_graph_ = on; }

    std::vector<CrtLabels> get_outputs(hipStream_t st) {
        bind_device(dev_, st, "HipEvaluator.get_outputs");
        std::vector<CrtLabels> out(B_);
        stage_outputs(st);
        for (int b = 0; b < B_; ++b)
            for (int j = 0; j < k_; ++j) {
                const int q = out_mod_[j];
                Labels L(q, Nout_);
                const int n = L.n;
                for (i64 e = 0; e < Nout_; ++e)
                    for (int c = 0; c < n; ++c) L.c[e * n + c] = out_stage_[j][(static_cast<i64>(b) * n + c) * Nout_ + e];
                out[b].push_back(std::move(L));
            }
        return out;
    }

    void set_profile(bool on) {
        profile_ = on;
        if (on && ev_.empty()) {
            bind_device(dev_, nullptr, "HipEvaluator.set_profile");
            ev_.resize(ops_.size() + 1);
            for (auto& e : ev_) HIPCHECK(hipEventCreate(&e));
        }
    }
    std::vector<std::pair<std::string, double>> op_times() const {
        std::vector<std::pair<std::string, double>> r;
        if (!profile_) return r;
        for (size_t i = 0; i < ops_.size(); ++i) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]);
            r.emplace_back(op_names_[i], ms);
        }
        return r;
    }

   private:
    std::shared_ptr<std::atomic<bool>> alive_ = std::make_shared<std::atomic<bool>>(true);
    // ------------------------------------------------------------ helpers
    template <typename T>
    T* dalloc(size_t count) {
        void* p = nullptr;
        size_t bytes = std::max<size_t>(count * sizeof(T), 64);
        HIPCHECK(hipMalloc(&p, bytes));
        allocs_.push_back(p);
        dev_bytes_ += bytes;
        return static_cast<T*>(p);
    }
    template <typename T>
    T* upload(const T* host, size_t count) {
        T* d = dalloc<T>(count);
        HIPCHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    // a model array into device memory: device-to-device (or peer) when the GPU
    // garbler left it in HBM and nobody has fetched (and possibly edited) a host copy
    static void copy_in(uint8_t* dst, const Array& a, hipStream_t st) {
        if (a.in_slot) return;  // skeleton model: the garbler wrote these bytes into this slot (IPC sink)
        if (a.device_resident() && a.device_ptr() == dst) return;  // garbled straight into this slot (sink)
        if (a.device_resident() && !a.dev->host)
            HIPCHECK(hipMemcpyAsync(dst, a.device_ptr(), a.nbytes, hipMemcpyDefault, st));
        else  // pageable host source: staged before the call returns
            HIPCHECK(hipMemcpyAsync(dst, a.ptr<uint8_t>(), a.nbytes, hipMemcpyHostToDevice, st));
    }
    // a per-GC small constant of `bytes` at dst0 + b * stride for slot b, filled on the host by `fill`
    void add_small(uint8_t* dst0, size_t stride, size_t bytes, std::function<void(const GarbledModel&, uint8_t*)> fill) {
        SmallLoad c;
        c.off = small_bytes_;
        c.dst0 = dst0;
        c.stride = stride;
        c.bytes = bytes;
        c.fill = std::move(fill);
        small_bytes_ += (bytes + 15) / 16 * 16;
        small_.push_back(std::move(c));
    }
    // after build(): staging buffers and the device descriptor table of the small constants
    void finish_small() {
        if (small_.empty()) return;
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&small_h_), small_bytes_));
        host_allocs_.push_back(small_h_);
        small_d_ = dalloc<uint8_t>(small_bytes_);
        std::vector<ScatterDesc> d;
        for (const auto& c : small_) d.push_back(ScatterDesc{c.off, c.dst0, c.stride, c.bytes});
        small_desc_ = upload(d.data(), d.size());
    }
    // one device buffer holding array `name` of layer li of every GC slot
    const u128* upload_tables(size_t li, const std::string& name) {
        const size_t nb = tmpl_->layers[li].arr(name).nbytes;
        if (stream_) return stream_table(li, name, nb);
        uint8_t* d = dalloc<uint8_t>(nb * B_);
        arena_[{li, name}] = {d, nb};
        loaders_.push_back([this, d, nb, li, name](int b, const GarbledModel& m) {
            const Array& a = m.layers[li].arr(name);
            DASH_CHECK(a.nbytes == nb, "table size mismatch across batch");
            copy_in(d + nb * b, a, load_st_);
        });
        table_bytes_ += nb * B_;
        return reinterpret_cast<const u128*>(d);
    }
    // Streamed tables (stream_tables): every GC's copy of the array lives in pinned host memory; the layer's
    // tables of all B slots are copied into one of three rotating HBM windows on a copy stream one layer
    // ahead of their use (stage_layer), so the device holds at most three layers of tables. For models (or
    // batches) whose tables exceed the HBM pool; the reference uploads every table at load (sign_gadget.h
    // cuda_move, 708-734). Three windows because a joint rescale's op runs in the next layer, reading its
    // own layer's tables: layer x's window is reused by layer x + 3 only after layer x + 1 has finished.
    const u128* stream_table(size_t li, const std::string& name, size_t nb) {
        const size_t span = (nb * B_ + 255) / 256 * 256;
        DASH_CHECK(woff_[li] + span <= win_bytes_, "streamed tables: layer window overflow");
        uint8_t* d = win_[li % 3] + woff_[li];
        woff_[li] += span;
        uint8_t* h = nullptr;
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&h), std::max<size_t>(16, nb * B_)));
        host_allocs_.push_back(h);
        stabs_[li].push_back(StreamTab{d, h, nb});
        loaders_.push_back([h, nb, li, name](int b, const GarbledModel& m) {
            const Array& a = m.layers[li].arr(name);
            DASH_CHECK(a.nbytes == nb, "table size mismatch across batch");
            if (a.device_resident() && !a.dev->host)
                HIPCHECK(hipMemcpy(h + nb * b, a.device_ptr(), nb, hipMemcpyDeviceToHost));
            else
                std::memcpy(h + nb * b, a.ptr<uint8_t>(), nb);
        });
        table_bytes_ += nb * B_;
        return reinterpret_cast<const u128*>(d);
    }
    // Op at the start of layer li's ops: layer li - 2 is done (its window may be refilled), layer li + 1's
    // tables go up on the copy stream (layer 0's too, at li = 0), and the evaluation waits for layer li's.
    void stage_layer(size_t li, hipStream_t st) {
        if (li >= 2) HIPCHECK(hipEventRecord(done_[li - 2], st));
        auto issue = [&](size_t x) {
            if (x >= stabs_.size() || stabs_[x].empty()) return;
            if (x >= 3) HIPCHECK(hipStreamWaitEvent(copy_st_, done_[x - 3], 0));
            else if (run_end_recorded_) HIPCHECK(hipStreamWaitEvent(copy_st_, run_end_, 0));  // the previous run's
            for (const auto& t : stabs_[x])
                HIPCHECK(hipMemcpyAsync(t.d, t.h, t.nb * B_, hipMemcpyHostToDevice, copy_st_));
            HIPCHECK(hipEventRecord(ready_[x], copy_st_));
        };
        if (li == 0) issue(0);
        issue(li + 1);
        if (!stabs_[li].empty()) HIPCHECK(hipStreamWaitEvent(st, ready_[li], 0));
    }
    void stage_end(hipStream_t st) {
        HIPCHECK(hipEventRecord(run_end_, st));
        run_end_recorded_ = true;
    }
    void init_streaming(const GarbledModel& m0) {
        const size_t L = m0.layers.size();
        size_t most = 256;
        for (const auto& l : m0.layers) {
            size_t s = 0;
            for (const auto& kv : l.a) s += (kv.second.nbytes * B_ + 255) / 256 * 256;
            most = std::max(most, s);
        }
        win_bytes_ = most;
        for (auto& w : win_) w = dalloc<uint8_t>(win_bytes_);
        woff_.assign(L, 0);
        stabs_.assign(L, {});
        ready_.resize(L);
        done_.resize(L);
        for (auto& e : ready_) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto& e : done_) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&run_end_, hipEventDisableTiming));
        HIPCHECK(hipStreamCreateWithFlags(&copy_st_, hipStreamNonBlocking));
        use_graph_ = false;  // the copy stream's waits on the previous run are issued per run
    }
    // all-zero device rows (the hardened encoding ships no constant labels: public-constant wires have label 0)
    const int16_t* zero_i16(size_t count) {
        int16_t* d = dalloc<int16_t>(count);
        HIPCHECK(hipMemset(d, 0, std::max<size_t>(count * sizeof(int16_t), 64)));
        return d;
    }
    const int16_t* upload_i16_rows(size_t li, const std::string& name) {
        const size_t nb = tmpl_->layers[li].arr(name).nbytes;
        uint8_t* d = dalloc<uint8_t>(nb * B_);
        add_small(d, nb, nb, [nb, li, name](const GarbledModel& m, uint8_t* h) {
            const Array& a = m.layers[li].arr(name);
            DASH_CHECK(a.nbytes == nb, "bias rows size mismatch across batch");
            std::memcpy(h, a.ptr<uint8_t>(), nb);
        });
        return reinterpret_cast<const int16_t*>(d);
    }
    // per-GC concatenated residue labels from model consts ("up.j", "down.s.j", "Z.p")
    const int16_t* upload_const_rows(const std::function<std::string(int)>& name_of) {
        if (hard_) return zero_i16(static_cast<size_t>(B_) * lab_stride_);
        int16_t* d = dalloc<int16_t>(static_cast<size_t>(B_) * lab_stride_);
        std::vector<std::string> names;
        for (int j = 0; j < k_; ++j) names.push_back(name_of(j));
        const int ls = lab_stride_, k = k_;
        std::vector<int> off(lab_off_, lab_off_ + k_), crt = crt_;
        add_small(reinterpret_cast<uint8_t*>(d), sizeof(int16_t) * ls, sizeof(int16_t) * ls,
                  [names, ls, k, off, crt](const GarbledModel& m, uint8_t* hb) {
            int16_t* h = reinterpret_cast<int16_t*>(hb);
            std::fill(h, h + ls, int16_t(0));
            for (int j = 0; j < k; ++j) {
                auto it = m.consts.find(names[j]);
                DASH_CHECK(it != m.consts.end(), "missing model constant " + names[j]);
                std::memcpy(&h[off[j]], it->second.ptr<int16_t>(), sizeof(int16_t) * nr_comps(crt[j]));
            }
        });
        return d;
    }
    CrtInfo crt_info(const std::vector<int>& mods) const {
        CrtInfo c{};
        c.k = static_cast<int>(mods.size());
        int s = 0;
        for (int j = 0; j < c.k; ++j) {
            c.p[j] = mods[j];
            c.n[j] = nr_comps(mods[j]);
            c.prefix[j] = s;
            s += mods[j];
        }
        c.sum = s;
        return c;
    }
    Act act_of(int which) const { return bufs_[which]; }
    void add_op(const std::string& name, std::function<void(hipStream_t)> f) {
        ops_.push_back(std::move(f));
        op_names_.push_back(name);
    }

    // sign gadget phases over `x` (N elements); results in sign scratch
    struct Sign {
        SignArgs a;
        int maxn;  // widest label of the carry chain (launch_sign_chain's template pick)
    };
    Sign make_sign(size_t li, const std::string& pre, const SignPlan& sp, i64 N, int relu, uint64_t sgate0 = 0,
                   uint64_t mgate0 = 0) {
        SignArgs a{};
        a.hard = hard_ ? 1 : 0;
        a.sgate0 = sgate0;
        a.mgate0 = mgate0;
        a.ny = ny_;
        a.ys = ys_;
        a.crt = crt_info(crt_);
        a.t = static_cast<int>(sp.mrs.size());
        DASH_CHECK(a.t <= kMaxMrs, "MRS base too long for the GPU path");
        for (int d = 0; d < a.t; ++d) a.mrs[d] = sp.mrs[d];
        a.nout = static_cast<int>(sp.out_mod.size());
        for (int o = 0; o < a.nout; ++o) a.out_mod[o] = sp.out_mod[o];
        a.N = N;
        a.B = B_;
        a.n_approx = sp.n_approx;
        a.fused = sp.fused ? 1 : 0;
        a.n_cast = tmpl_->layers[li].arr(pre + "s.cast2").shape[1];
        a.n_sign = sp.n_sign;
        a.approx = upload_tables(li, pre + "s.approx");
        a.cast1 = sp.has_cast1() ? upload_tables(li, pre + "s.cast1") : nullptr;
        a.cast2 = upload_tables(li, pre + "s.cast2");
        a.sign = upload_tables(li, pre + "s.sign");
        a.mrsP = mrsP_;
        a.hx = relu ? hx_ : nullptr;
        a.colx = relu ? colx_ : nullptr;
        a.outP = outP_;
        a.hs = hs_;
        a.cs = cs_;
        a.zc = zc_;
        a.zcol = zcol_;
        a.zc_stride = zstride_;
        a.relu = relu;
        a.csum = csum_;
        {
            int64_t c1 = 0;
            for (int d = a.t - 1; d >= 1; --d) {
                a.c1off[d] = c1;
                c1 += static_cast<int64_t>(k_ + 1) * a.mrs[d];
            }
            // a one-digit MRS base (t = 1) has no casts: the garbler stores a 1-entry placeholder row
            DASH_CHECK(c1 == a.n_cast || (c1 == 0 && a.n_cast <= 1), "cast row size does not match the MRS base");
        }
        int maxn = 0;
        const int k = k_;
        for (size_t d = 1; d < sp.mrs.size(); ++d) maxn = std::max(maxn, nr_comps((k + 1) * sp.mrs[d]));
        maxn = std::max(maxn, nr_comps(sp.mrs[0]));
        DASH_CHECK(maxn <= 64, "MRS moduli too small for the GPU sign chain (label width > 64)");
        return {a, maxn};
    }

    // ------------------------------------------------------------ planner
    // build() is the driver: constants, shape pass, buffers, one plan_<kind> per layer, output staging. What the
    // walk over the layers knows lives in a Walk on build()'s stack; nothing of it outlives build().
    struct Env {  // what almost every op needs besides its own arguments; captured by value
        const ModC* mc;
        AesGlobals ag;
        int B;
    };
    struct Caps {  // shape pass: buffer capacities in elements per GC, label widths, every layer's output size
        i64 maxN, maxSignN, maxPoolSlots, maxArgSlots;
        std::vector<int> widest;  // [j] widest label of residue j's buffer (projections change the moduli)
        std::vector<i64> outN;    // [slot] slot 0: the circuit input, slot li + 1: layer li's output
    };
    struct Walk {
        Env env;
        Caps caps;
        CrtInfo crt;            // of crt_
        int cur = 0;            // buffer index holding the current activation
        i64 N = 0;              // its elements per GC
        std::vector<int> mods;  // its moduli
        std::vector<int> keep;  // [slot] a later layer reads this output (Add, Concat, in_src): save_if_needed
        std::vector<i64> saved_n;  // [slot] elements and moduli of the copies in saved_
        std::vector<std::vector<int>> saved_mods;
        // a sign-producing rescale whose outputs the next layer's op writes in its own pass: a joint ReLU's
        // launch_rescale_relu_out or a joint Clip's launch_rescale_clip_out. At most one is pending.
        enum class Pending { none, relu, clip, leaky } pending = Pending::none;
        MrsArgs pending_a{};
        int nxt() const { return (cur + 1) % 2; }
    };
    // The one statement of a layer's output element count: the shape pass sizes the buffers with it and every
    // planner checks the N it leaves against it (set_out).
    static i64 out_elems(const GLayer& l, i64 N_in, const std::vector<i64>& outN) {
        switch (l.kind) {
            case K_DENSE: return l.param("out");
            case K_CONV: return ConvGeom(l).out_size();
            case K_CONVT: return ConvTGeom(l).out_size();
            case K_UPSAMPLE: return UpGeom(l.p).out_size();
            case K_GATHER: return static_cast<i64>(l.vec("idx").size());
            case K_BILINEAR: return BilinearGeom(l.p).out_size();
            case K_MAXPOOL: case K_SUMPOOL: return PoolGeom(l.p).out_size();
            case K_MAX: return 1;
            case K_ARGMAX: return l.param("P");
            case K_CONCAT: {
                i64 N = 0;
                for (i64 s : l.vec("srcs")) {
                    DASH_CHECK(s >= -1 && s + 1 < static_cast<i64>(outN.size()), "concat: bad source layer");
                    N += outN[s + 1];
                }
                return N;
            }
            case K_MULT: case K_MMULT: return N_in / 2;
            case K_MATMUL: return l.param("G", 1) * l.param("M") * l.param("N");
            default: return N_in;
        }
    }
    // a planner's last step: its output, N elements, is in buffer `buf` (w.nxt(), or w.cur for an in-place layer)
    void set_out(Walk& w, const GLayer& g, i64 N, int buf) const {
        DASH_CHECK(N == out_elems(g, w.N, w.caps.outN),
                   std::string("planner and shape pass disagree on the output size of ") + kind_name(g.kind));
        w.N = N;
        w.cur = buf;
    }
    template <typename A>
    void set_label_rows(A& a) const {  // DenseArgs, ConvArgs, RescaleArgs: the zero-label rows and their layout
        a.zero = zero_rows_;
        a.lab_stride = lab_stride_;
        for (int j = 0; j < k_; ++j) a.lab_off[j] = lab_off_[j];
    }
    // factor f of a RescalePlan: the residues it updates, their trans rows and the factor residue's hashes
    void set_active(RescaleArgs& ra, const RescalePlan& P, size_t f, const u128* trans) const {
        for (size_t q = 0; q < P.active[f].size(); ++q) {
            const int jj = P.active[f][q];
            ra.active[jj] = 1;
            ra.aidx[jj] = static_cast<int>(q);
            ra.inv[jj] = static_cast<int>(P.inv[f][q]);
        }
        ra.n_trans = P.n_trans;
        ra.trans = trans;
        ra.h0 = h0_;
        ra.col0 = col0_;
    }
    // scratch that only some layer kinds need, allocated by the first layer that does
    void ensure_mrs_ps(const Walk& w) {
        if (!mrs_ps_) mrs_ps_ = dalloc<u128>(static_cast<size_t>(B_) * std::max(1, k_ * (k_ - 1) / 2) * w.caps.maxSignN);
    }
    void ensure_ks(const Walk& w, int sides) {
        for (int side = 0; side < sides; ++side)
            if (!ks_[side]) ks_[side] = dalloc<u128>(static_cast<size_t>(B_) * w.caps.maxSignN);
    }
    // a PiecewiseLinear's sign labels, one buffer per kept breakpoint: sized by the model's largest count
    void ensure_kpwl(const Walk& w) {
        int mmax = 0;
        for (const GLayer& l : tmpl_->layers)
            if (l.kind == K_PWL)
                mmax = std::max(mmax, PwlPlan(crt_, l.param("s"), l.vec("T"), l.vec("A"), l.param("V")).m());
        for (int i = 0; i < mmax; ++i)
            if (!kpwl_[i]) kpwl_[i] = dalloc<u128>(static_cast<size_t>(B_) * w.caps.maxSignN);
    }
    // a MatMul's operand keys and colours ([B][k][G M T] and [B][k][G T N]): sized by the model's largest operands
    void ensure_matmul() {
        i64 nx = 0, ny = 0;
        for (const GLayer& l : tmpl_->layers)
            if (l.kind == K_MATMUL) {
                nx = std::max(nx, l.param("G", 1) * l.param("M") * l.param("T"));
                ny = std::max(ny, l.param("G", 1) * l.param("T") * l.param("N"));
            }
        if (!mm_kx_) {
            mm_kx_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * nx);
            mm_cx_ = dalloc<uint16_t>(static_cast<size_t>(B_) * k_ * nx);
            mm_ky_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * ny);
            mm_cy_ = dalloc<uint16_t>(static_cast<size_t>(B_) * k_ * ny);
        }
    }
    // The exact mixed-radix sign's chain (mode 1, gadgets.h SignMrsPlan) over N elements with layer li's table
    // `table`: a ReLU's (ny = ny_: the sign label's y-row pads), or with the label itself kept in `ks` and ny = 0
    // for a Clip's two signs, a joint Clip's upper sign and an ArgMax level.
    MrsArgs mrs_sign_args(const Walk& w, size_t li, const std::string& table, i64 N, uint64_t gate0, uint64_t rgate0,
                          int ny, u128* ks) {
        const SignMrsPlan P(crt_);
        MrsArgs a{};
        a.crt = w.crt;
        a.N = N;
        a.n_tab = tmpl_->layers[li].arr(table).shape[1];
        a.tab = upload_tables(li, table);
        for (int i = 0; i + 1 < k_; ++i) a.dig_off[i] = P.dig_off[i];
        ensure_mrs_ps(w);
        a.ps = mrs_ps_;
        a.mode = 1;
        a.hs = hs_;
        a.cs = cs_;
        a.gate0 = gate0;
        a.rgate0 = rgate0;
        a.ny = ny;
        a.ys = ys_;
        a.ks = ks;
        return a;
    }
    // the multiply of a ReLU whose sign label is already in hs_ / cs_ (joint and mixed-radix-sign ReLUs)
    SignArgs joint_sign_args(const Walk& w, size_t li, i64 N) const {
        SignArgs sa{};
        sa.crt = w.crt;
        sa.N = N;
        sa.B = B_;
        sa.hx = hx_;
        sa.colx = colx_;
        sa.hs = hs_;
        sa.cs = cs_;
        sa.hard = hard_ ? 1 : 0;
        sa.mgate0 = gate_base(li + 1, 2);
        sa.ny = ny_;
        sa.ys = ys_;
        return sa;
    }
    BEArgs be_args(const Walk& w, const BEPlan& be, size_t li, const std::string& table, i64 N, uint64_t gate0) {
        BEArgs ba{};
        ba.E = static_cast<int>(be.moduli.size());
        ba.nonext = be.nonext;
        std::vector<int> idx(ba.E);
        for (int i = 0; i < ba.E; ++i) idx[be.pos_of[i]] = i;
        for (int i = 0; i < ba.E; ++i) {
            ba.swapped[i] = be.swapped[i];
            ba.src[i] = idx[i];
        }
        for (int i = 0; i + 1 < ba.E; ++i)
            for (size_t jj = 0; jj < be.inv_partial[i].size(); ++jj) ba.inv[i][jj] = static_cast<int>(be.inv_partial[i][jj]);
        ba.nextra = static_cast<int>(be.extra.size());
        for (int xi = 0; xi < ba.nextra; ++xi) {
            ba.extra_res[xi] = be.extra_idx[xi];
            ba.extra_pos[xi] = be.pos_of[be.extra_idx[xi]];
            ba.invv[xi] = static_cast<int>(pmod(-be.invv[xi], be.moduli[be.extra_idx[xi]]));
        }
        ba.N = N;
        ba.n_tab = be.n_tab;
        ba.tab = upload_tables(li, table);
        if (!be_work_) be_work_ = dalloc<int16_t>(static_cast<size_t>(B_) * k_ * 128 * w.caps.maxN);
        ba.work = be_work_;
        ba.hard = hard_ ? 1 : 0;
        ba.gate0 = gate0;
        return ba;
    }

    void build();
    void upload_constants();
    Caps shape_pass() const;
    void alloc_buffers(const Caps& c);
    void save_if_needed(Walk& w, size_t slot);
    void restore_in_src(Walk& w, const GLayer& g);
    void alloc_output_staging(const Walk& w);
    void plan_dense(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_conv(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_convt(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_upsample(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_gather(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_bilinear(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_relu(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_clip(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_sign(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_rescale(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_rescale_mrs(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_rescale_clip(Walk& w, size_t li, MrsArgs a, const std::string& lname);
    void plan_rescale_legacy(Walk& w, size_t li, i64 iters, Act x, const std::string& lname);
    void plan_rescale_redash(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_max(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_argmax(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_sumpool(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_add(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_concat(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_proj(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_mult(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_mul(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_matmul(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_leaky(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_pwl(Walk& w, size_t li, const GLayer& g, const std::string& lname);
    void plan_base_ext(Walk& w, size_t li, const GLayer& g, const std::string& lname);

    std::shared_ptr<GarbledModel> tmpl_;  // build() only
    ModelHeader tmpl_h_;
    bool hard_ = false;     // the template's hardened flag (ModelHeader::hardened); every loaded GC must match
    int ny_ = 0;            // y-row pad slots of a ReLU's sign label: k entries + ceil(k / 8) mini pads
    u128* ys_ = nullptr;    // [B][ny][maxSignN] y-row pads (hardened ReLU sign labels)
    size_t tmpl_nlayers_ = 0;
    bool mfma_;
    // streamed tables (stream_table / stage_layer)
    bool stream_ = false;
    struct StreamTab {
        uint8_t* d;  // window address of slot 0 ([B][nb])
        uint8_t* h;  // pinned host copy ([B][nb])
        size_t nb;
    };
    uint8_t* win_[3] = {};
    size_t win_bytes_ = 0;
    std::vector<size_t> woff_;
    std::vector<std::vector<StreamTab>> stabs_;
    hipStream_t copy_st_ = nullptr;
    std::vector<hipEvent_t> ready_, done_;
    hipEvent_t run_end_ = nullptr;
    bool run_end_recorded_ = false;
    std::vector<std::function<void(int, const GarbledModel&)>> loaders_;
    struct SmallLoad {
        size_t off = 0;
        uint8_t* dst0 = nullptr;
        size_t stride = 0, bytes = 0;
        std::function<void(const GarbledModel&, uint8_t*)> fill;
    };
    std::vector<SmallLoad> small_;
    size_t small_bytes_ = 0;
    uint8_t* small_h_ = nullptr;
    uint8_t* small_d_ = nullptr;
    const ScatterDesc* small_desc_ = nullptr;
    hipStream_t load_st_ = nullptr;
    std::mutex load_mu_;  // load(): the staging blocks and load stream above are shared by every slot
    std::map<std::pair<size_t, std::string>, std::pair<uint8_t*, size_t>> arena_;  // (layer, table) -> [B][nb]
    std::vector<int> loaded_;
    int dev_ = 0, B_ = 1, k_ = 0;
    std::vector<int> crt_, out_mod_;
    i64 N0_ = 0, Nout_ = 0;
    std::vector<void*> allocs_, host_allocs_;
    size_t dev_bytes_ = 0, table_bytes_ = 0;
    std::vector<std::function<void(hipStream_t)>> ops_;
    std::vector<std::string> op_names_;
    bool profile_ = false;
    std::vector<hipEvent_t> ev_;
    Act bufs_[4]{};  // ping-pong activation buffers (+ scratch)
    Act final_{};
    std::vector<int16_t*> in_stage_;
    std::vector<act_t*> out_stage_;
    std::vector<void*> out_stage_dev_;  // device addresses of the mapped out_stage_ buffers
    bool out_stage_mapped_ = true;
    int16_t* in16_dev_[kMaxRes] = {};  // device int16 copy of the host-encoded inputs (uncompressed input path)
    u128* in_comp_stage_ = nullptr;
    bool use_graph_ = [] {
        const char* e = std::getenv("DASH_HIP_GRAPH");
        return !(e && e[0] == '0');
    }();
    hipGraphExec_t gexec_ = nullptr;
    hipStream_t gstream_ = nullptr;
    long runs_ = 0;
    u128* in_comp_dev_ = nullptr;
    // constants
    ModC* mc_ = nullptr;
    AesGlobals aes_{};
    int lab_stride_ = 0;
    int lab_off_[kMaxRes]{};
    int* d_lab_off_ = nullptr;
    const int16_t* zero_rows_ = nullptr;
    const int16_t* up_rows_ = nullptr;
    u128* mrs_ps_ = nullptr;  // mixed-radix rescale chain scratch (allocated by the first such layer)
    u128 *mm_kx_ = nullptr, *mm_ky_ = nullptr;  // a MatMul's operand keys and colours (ensure_matmul)
    uint16_t *mm_cx_ = nullptr, *mm_cy_ = nullptr;
    u128* kpwl_[kPwlMax] = {};  // [B][maxSignN] a PiecewiseLinear's sign labels (allocated by the first such layer)
    u128* ks_[2] = {nullptr, nullptr};  // [B][maxSignN] a Clip's two sign labels (allocated by the first Clip)
    // ArgMax scratch (allocated by the first ArgMax): candidate values / index labels of the odd levels, the value
    // and index differences; the index gates' garbler-half pads and colours
    Act amb_[4] = {};
    u128* am_hi_ = nullptr;
    uint16_t* am_coli_ = nullptr;
    const u128* zc_ = nullptr;
    const u128* zh_ = nullptr;
    const uint16_t* zcol_ = nullptr;
    int zstride_ = 0;
    // scratch
    u128 *mrsP_ = nullptr, *hx_ = nullptr, *outP_ = nullptr, *hs_ = nullptr, *h0_ = nullptr;
    uint16_t *colx_ = nullptr, *col0_ = nullptr;
    uint8_t* cs_ = nullptr;
    int16_t* csum_ = nullptr;
    int16_t* be_work_ = nullptr;
    std::vector<std::vector<act_t*>> saved_;  // residual-add sources
};

void HipEvaluator::build() {
    const GarbledModel& m0 = *tmpl_;
    const size_t L = m0.layers.size();
    hard_ = m0.h.hardened != 0;
    ny_ = k_ + (k_ + 7) / 8;
    upload_constants();
    N0_ = 1;
    for (auto d : m0.h.in_dims) N0_ *= d;
    Walk w{Env{mc_, aes_, B_}, shape_pass(), crt_info(crt_)};
    alloc_buffers(w.caps);

    w.N = N0_;
    w.mods = crt_;
    w.keep.assign(L + 1, 0);
    for (auto& l : m0.layers) {
        if (l.kind == K_ADD) w.keep[l.param("src") + 1] = 1;
        if (l.kind == K_MUL && !l.param("sq", 0)) {
            const i64 s = l.param("src");
            DASH_CHECK(s >= -1 && s < static_cast<i64>(L), "mul: bad source layer");
            w.keep[s + 1] = 1;
        }
        if (l.kind == K_MATMUL) {
            const i64 s = l.param("src");
            DASH_CHECK(s >= -1 && s < static_cast<i64>(L), "matmul: bad source layer");
            w.keep[s + 1] = 1;
        }
        if (l.kind == K_CONCAT)
            for (i64 s : l.vec("srcs")) w.keep[s + 1] = 1;
        if (l.p.count("in_src")) w.keep[l.param("in_src") + 1] = 1;
    }
    saved_.assign(L + 1, {});
    w.saved_n.assign(L + 1, 0);
    w.saved_mods.assign(L + 1, {});
    save_if_needed(w, 0);
    if (stream_) init_streaming(m0);

    for (size_t li = 0; li < L; ++li) {
        const GLayer& g = m0.layers[li];
        if (stream_) add_op("stage", [this, li](hipStream_t st) { stage_layer(li, st); });
        const std::string lname = std::string(kind_name(g.kind)) + "#" + std::to_string(li);
        // a Gather reads its in_src source in place (plan_gather): no copy back into the current buffer
        if (g.p.count("in_src") && g.kind != K_GATHER) restore_in_src(w, g);
        switch (g.kind) {
            case K_FLATTEN: break;
            case K_DENSE: plan_dense(w, li, g, lname); break;
            case K_CONV: plan_conv(w, li, g, lname); break;
            case K_CONVT: plan_convt(w, li, g, lname); break;
            case K_UPSAMPLE: plan_upsample(w, li, g, lname); break;
            case K_GATHER: plan_gather(w, li, g, lname); break;
            case K_BILINEAR: plan_bilinear(w, li, g, lname); break;
            case K_RELU: plan_relu(w, li, g, lname); break;
            case K_CLIP: plan_clip(w, li, g, lname); break;
            case K_SIGN: plan_sign(w, li, g, lname); break;
            case K_RESCALE: plan_rescale(w, li, g, lname); break;
            case K_MAXPOOL: case K_MAX: plan_max(w, li, g, lname); break;
            case K_ARGMAX: plan_argmax(w, li, g, lname); break;
            case K_SUMPOOL: plan_sumpool(w, li, g, lname); break;
            case K_ADD: plan_add(w, li, g, lname); break;
            case K_CONCAT: plan_concat(w, li, g, lname); break;
            case K_PROJ: plan_proj(w, li, g, lname); break;
            case K_MULT: case K_MMULT: plan_mult(w, li, g, lname); break;
            case K_MUL: plan_mul(w, li, g, lname); break;
            case K_MATMUL: plan_matmul(w, li, g, lname); break;
            case K_LEAKY: plan_leaky(w, li, g, lname); break;
            case K_PWL: plan_pwl(w, li, g, lname); break;
            case K_BASEEXT: plan_base_ext(w, li, g, lname); break;
            default:
                throw std::runtime_error(std::string("dash: HIP evaluator cannot run layer kind ") + kind_name(g.kind));
        }
        save_if_needed(w, li + 1);
    }
    // a deferred rescale's output kernel is the next layer's op: left pending, it would never run
    DASH_CHECK(w.pending == Walk::Pending::none, "planner: a deferred rescale output was never planned");
    if (stream_) add_op("stage_end", [this](hipStream_t st) { stage_end(st); });
    alloc_output_staging(w);
    finish_small();
    HIPCHECK(hipDeviceSynchronize());
}

// ---- global constants
void HipEvaluator::upload_constants() {
    const GarbledModel& m0 = *tmpl_;
    const int maxmod = m0.h.max_mod;
    std::vector<ModC> mc(maxmod + 1);
    for (int q = 2; q <= maxmod; ++q) mc[q] = make_modc(q);
    DASH_CHECK(modk_table_ok(), "dev::ModK constants differ from the ModC table");  // the constant-modulus kernels
    mc_ = upload(mc.data(), mc.size());
    auto te = make_te0();
    auto rk = fixed_round_key_words();
    aes_.te0 = upload(te.data(), te.size());
    aes_.rk = upload(rk.data(), rk.size());
    for (int j = 0; j < k_; ++j) {
        lab_off_[j] = lab_stride_;
        lab_stride_ += nr_comps(crt_[j]);
    }
    d_lab_off_ = upload(lab_off_, k_);
    prepare_zmap(crt_info(crt_));  // VALU dense / conv block lookup, built here (not under a graph capture)
    zero_rows_ = upload_const_rows([&](int j) { return "Z." + std::to_string(crt_[j]); });
    // compressed zero labels + colors for every modulus (carry init)
    zstride_ = maxmod + 1;
    {
        u128* dzc = dalloc<u128>(static_cast<size_t>(B_) * zstride_);
        u128* dzh = dalloc<u128>(static_cast<size_t>(B_) * zstride_);
        uint16_t* dzcol = dalloc<uint16_t>(static_cast<size_t>(B_) * zstride_);
        zc_ = dzc;
        zh_ = dzh;
        zcol_ = dzcol;
        const int zs = zstride_;
        // compressed zero labels, their hashes and colors: one fill writes all three staging blocks (the zc
        // block's fill computes them; the two followers' fills are no-ops on the same pass)
        auto zfill = [zs, maxmod](const GarbledModel& m, u128* zc, u128* zh, uint16_t* zcol) {
            std::fill(zc, zc + zs, u128(0));
            std::fill(zh, zh + zs, u128(0));
            std::fill(zcol, zcol + zs, uint16_t(0));
            LabelBank Z = m.zero_bank();
            for (int q = 2; q <= maxmod; ++q) {
                if (Z.lab[q].empty()) continue;
                zc[q] = compress(Z.lab[q].data(), mod_info(q));
                zh[q] = hash(zc[q]);
                zcol[q] = static_cast<uint16_t>(Z.lab[q][0]);
            }
        };
        const size_t zcb = sizeof(u128) * zs, zcolb = sizeof(uint16_t) * zs;
        const size_t zoff = small_bytes_;  // the three blocks are staged back to back (16-B rounded)
        const size_t zhoff = zoff + (zcb + 15) / 16 * 16, zcoloff = zhoff + (zcb + 15) / 16 * 16;
        add_small(reinterpret_cast<uint8_t*>(dzc), zcb, zcb, [zfill, zoff, zhoff, zcoloff](const GarbledModel& m, uint8_t* h) {
            zfill(m, reinterpret_cast<u128*>(h), reinterpret_cast<u128*>(h + (zhoff - zoff)),
                  reinterpret_cast<uint16_t*>(h + (zcoloff - zoff)));
        });
        add_small(reinterpret_cast<uint8_t*>(dzh), zcb, zcb, [](const GarbledModel&, uint8_t*) {});
        add_small(reinterpret_cast<uint8_t*>(dzcol), zcolb, zcolb, [](const GarbledModel&, uint8_t*) {});
    }
    bool any_rescale = false;
    for (auto& l : m0.layers) any_rescale |= (l.kind == K_RESCALE && l.param("mode", 0) != 2);  // mode 2: no shift labels
    if (any_rescale) up_rows_ = upload_const_rows([&](int j) { return "up." + std::to_string(j); });
}

// ---- shape pass: buffer capacities. Output sizes come from out_elems; the scratch capacities are this pass's own.
HipEvaluator::Caps HipEvaluator::shape_pass() const {
    Caps c{N0_, 1, 1, 0, std::vector<int>(k_, 0), {N0_}};
    for (int j = 0; j < k_; ++j) c.widest[j] = nr_comps(crt_[j]);
    i64 N = N0_;
    for (auto& l : tmpl_->layers) {
        if (l.p.count("in_src")) N = c.outN.at(l.param("in_src") + 1);
        const i64 No = out_elems(l, N, c.outN);
        switch (l.kind) {
            case K_RELU: case K_SIGN: case K_RESCALE: case K_CLIP: case K_LEAKY: case K_PWL:
                c.maxSignN = std::max(c.maxSignN, N);
                break;
            case K_MAXPOOL: {
                PoolGeom G(l.p);
                c.maxPoolSlots = std::max(c.maxPoolSlots, No * G.kh * G.kw);
                c.maxSignN = std::max(c.maxSignN, No * G.kh * G.kw);
                break;
            }
            case K_MAX:
                c.maxPoolSlots = std::max(c.maxPoolSlots, N);
                c.maxSignN = std::max(c.maxSignN, N);
                break;
            case K_ARGMAX: {  // the widest level: floor(K / 2) pair operations, ceil(K / 2) slots behind it
                const i64 K = l.param("K");
                c.maxSignN = std::max(c.maxSignN, (K / 2) * No);
                c.maxArgSlots = std::max(c.maxArgSlots, ((K + 1) / 2) * No);
                break;
            }
            case K_PROJ: {
                const auto& om = l.vec("out_mod");
                for (int j = 0; j < k_; ++j) c.widest[j] = std::max(c.widest[j], nr_comps(static_cast<int>(om[j])));
                break;
            }
            default: break;
        }
        N = No;
        c.maxN = std::max(c.maxN, N);
        c.outN.push_back(N);
    }
    return c;
}

void HipEvaluator::alloc_buffers(const Caps& c) {
    const i64 cap = std::max(c.maxN, c.maxPoolSlots), maxSignN = c.maxSignN;
    for (int bi = 0; bi < 4; ++bi) {
        bufs_[bi].N = 0;
        for (int j = 0; j < k_; ++j) {
            // + 64 B: the MFMA dense kernel reads whole 16-byte k slices past the last column's end
            const size_t count = static_cast<size_t>(B_) * c.widest[j] * cap + 64;
            bufs_[bi].p[j] = dalloc<act_t>(count);
            // defined contents before any input is staged (serving primes the hipGraph with an unencoded run)
            HIPCHECK(hipMemset(bufs_[bi].p[j], 0, count * sizeof(act_t)));
        }
    }
    int tmax = std::max<int>(1, static_cast<int>(tmpl_->h.mrs.size()));
    mrsP_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * tmax * maxSignN);
    hx_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * maxSignN);
    csum_ = dalloc<int16_t>(static_cast<size_t>(B_) * tmax * kCsumComps * maxSignN);
    colx_ = dalloc<uint16_t>(static_cast<size_t>(B_) * k_ * maxSignN);
    outP_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * maxSignN);
    hs_ = dalloc<u128>(static_cast<size_t>(B_) * maxSignN);
    if (hard_) ys_ = dalloc<u128>(static_cast<size_t>(B_) * ny_ * maxSignN);
    cs_ = dalloc<uint8_t>(static_cast<size_t>(B_) * maxSignN);
    h0_ = dalloc<u128>(static_cast<size_t>(B_) * c.maxN);
    col0_ = dalloc<uint16_t>(static_cast<size_t>(B_) * c.maxN);
    for (int j = 0; j < k_; ++j) {
        int16_t* p = nullptr;
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(int16_t) * B_ * nr_comps(crt_[j]) * N0_));
        host_allocs_.push_back(p);
        in_stage_.push_back(p);
    }
}

// a copy of the current activation for the later layers that read output `slot` (w.keep)
void HipEvaluator::save_if_needed(Walk& w, size_t slot) {
    if (!w.keep[slot]) return;
    std::vector<act_t*> s;
    for (int j = 0; j < k_; ++j) {
        const size_t bytes = sizeof(act_t) * B_ * nr_comps(w.mods[j]) * w.N;
        act_t* d = dalloc<act_t>(bytes / sizeof(act_t));
        act_t* src = bufs_[w.cur].p[j];
        add_op("save", [d, src, bytes](hipStream_t st) { HIPCHECK(hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToDevice, st)); });
        s.push_back(d);
    }
    saved_[slot] = s;
    w.saved_n[slot] = w.N;
    w.saved_mods[slot] = w.mods;
}

// layer reads an earlier output (projection shortcut): restore it into the current buffer
void HipEvaluator::restore_in_src(Walk& w, const GLayer& g) {
    const i64 src = g.param("in_src");
    const auto& sv = saved_[src + 1];
    DASH_CHECK(!sv.empty(), "in_src source not saved");
    w.N = w.saved_n[src + 1];
    w.mods = w.saved_mods[src + 1];
    for (int j = 0; j < k_; ++j) {
        const size_t bytes = sizeof(act_t) * B_ * nr_comps(w.mods[j]) * w.N;
        act_t* d = bufs_[w.cur].p[j];
        const act_t* sp = sv[j];
        add_op("restore", [d, sp, bytes](hipStream_t st) {
            HIPCHECK(hipMemcpyAsync(d, sp, bytes, hipMemcpyDeviceToDevice, st));
        });
    }
}

void HipEvaluator::alloc_output_staging(const Walk& w) {
    final_ = act_of(w.cur);
    Nout_ = w.N;
    out_mod_ = w.mods;
    for (int j = 0; j < k_; ++j) {
        act_t* p = nullptr;
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(act_t) * B_ * nr_comps(w.mods[j]) * std::max<i64>(Nout_, 1)));
        host_allocs_.push_back(p);
        out_stage_.push_back(p);
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess || !dp) {
            (void)hipGetLastError();
            out_stage_mapped_ = false;
        }
        out_stage_dev_.push_back(dp);
    }
}

void HipEvaluator::plan_dense(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    DenseArgs a{};
    a.crt = w.crt;
    a.K = g.param("in");
    a.O = g.param("out");
    const i64 ch = g.param("channel_tf", 0);
    const Array& wt_src = g.arr("w");
    for (int j = 0; j < k_; ++j) {
        const int p = crt_[j];
        std::vector<int16_t> wt(static_cast<size_t>(a.K * a.O));
        std::vector<int32_t> zc(a.O, 0);
        for (i64 o = 0; o < a.O; ++o)
            for (i64 i = 0; i < a.K; ++i) {
                const int v = static_cast<int>(wt_src.ptr<i64>()[o * a.K + i] % p);
                wt[i * a.O + o] = static_cast<int16_t>(v);
                if (v == 0) ++zc[o];
            }
        a.w[j] = upload(wt.data(), wt.size());
        a.zc[j] = upload(zc.data(), zc.size());
        a.bias[j] = hard_ ? zero_i16(static_cast<size_t>(B_) * a.O * nr_comps(p))
                          : upload_i16_rows(li, arr_name("bias.", j, ""));
    }
    // MFMA path: centered int8 weights [O][Kpad], channel_tf folded into the column order
    a.Kpad = static_cast<int>((a.K + 63) / 64 * 64);
    bool mfma_ok = mfma_ && a.K < (1 << 17);  // 127 * 127 * K fits the int32 accumulator
    for (int j = 0; j < k_; ++j) mfma_ok = mfma_ok && crt_[j] <= 255;
    for (int j = 0; j < k_; ++j) {
        a.w8[j] = nullptr;
        if (!mfma_ok) continue;
        const int p = crt_[j];
        std::vector<int8_t> w8(static_cast<size_t>(a.O) * a.Kpad, 0);
        for (i64 o = 0; o < a.O; ++o)
            for (i64 i = 0; i < a.K; ++i) {
                const int v = static_cast<int>(wt_src.ptr<i64>()[o * a.K + i] % p);
                const i64 s = ch > 0 ? dense_src(i, a.K, ch) : i;
                w8[static_cast<size_t>(o) * a.Kpad + s] = static_cast<int8_t>(v > p / 2 ? v - p : v);
            }
        a.w8[j] = upload(w8.data(), w8.size());
    }
    set_label_rows(a);
    if (ch > 0) {
        std::vector<int32_t> src(a.K);
        for (i64 i = 0; i < a.K; ++i) src[i] = static_cast<int32_t>(dense_src(i, a.K, ch));
        a.src = upload(src.data(), src.size());
    }
    Act x = act_of(w.cur), y = act_of(w.nxt());
    x.N = w.N;
    y.N = a.O;
    const int B = B_;
    add_op(lname, [a, x, y, B](hipStream_t st) { launch_dense(a, x, y, B, st); });
    set_out(w, g, a.O, w.nxt());
}

void HipEvaluator::plan_conv(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    ConvGeom G(g);
    ConvArgs a{};
    a.crt = w.crt;
    a.C = static_cast<int>(G.C); a.H = static_cast<int>(G.H); a.W = static_cast<int>(G.W);
    a.F = static_cast<int>(G.F); a.kh = static_cast<int>(G.kh); a.kw = static_cast<int>(G.kw);
    a.sh = static_cast<int>(G.sh); a.sw = static_cast<int>(G.sw);
    a.ph = static_cast<int>(G.ph); a.pw = static_cast<int>(G.pw);
    a.OH = static_cast<int>(G.OH); a.OW = static_cast<int>(G.OW);
    a.dh = static_cast<int>(G.dh); a.dw = static_cast<int>(G.dw);
    const i64 K = G.K();
    a.use_mfma = mfma_ ? 1 : 0;
    a.groups = static_cast<int>(G.g);
    if (G.g > 1) {
        // grouped conv: the byte-stencil kernel, no MFMA plan
        a.use_mfma = 0;
        for (int j = 0; j < k_; ++j) {
            const u64 pm = static_cast<u64>(crt_[j] - 1);
            DASH_CHECK(crt_[j] <= kActMaxModulus, "grouped conv: residue modulus above 255");
            DASH_CHECK(static_cast<u64>(K) * pm * pm < (1ull << 32),
                       "grouped conv: (C/g)*kh*kw*(p-1)^2 must stay below 2^32 (32-bit accumulator)");
        }
        DASH_CHECK(conv_grp_geometry(a) > 0, "grouped conv: one output row of a group exceeds 64 KiB of LDS");
    } else {
        // LDS-image kernel geometry: 64-channel chunks, row bands that fit the LDS budget
        conv_layer_plan(a, mfma_ && conv_img_enabled());
    }
    a.img_off[0] = 0;
    for (int j = 0; j < k_; ++j) a.img_off[j + 1] = a.img_off[j] + static_cast<i64>(B_) * w.crt.n[j];
    const Array& wt = g.arr("w");
    for (int j = 0; j < k_; ++j) {
        const int p = crt_[j];
        const bool grp = G.g > 1;  // k_conv_grp reads its own image (wg) only
        std::vector<int16_t> wm(grp ? 0 : static_cast<size_t>(G.F * K));
        std::vector<int8_t> w8(grp ? 0 : static_cast<size_t>(G.F) * a.Kpad, 0);
        std::vector<int32_t> zc(G.F, 0);
        for (i64 f = 0; f < G.F; ++f)
            for (i64 q = 0; q < K; ++q) {
                const int v = static_cast<int>(wt.ptr<i64>()[f * K + q] % p);
                if (v == 0) ++zc[f];
                if (grp) continue;
                wm[f * K + q] = static_cast<int16_t>(v);
                w8[f * a.Kpad + q] = static_cast<int8_t>(v > p / 2 ? v - p : v);
            }
        a.w[j] = grp ? nullptr : upload(wm.data(), wm.size());
        a.w8[j] = (mfma_ && p <= 255 && !grp) ? upload(w8.data(), w8.size()) : nullptr;
        a.wg[j] = nullptr;
        if (grp) {
            const std::vector<uint32_t> wg =
                conv_grp_weights(wt.ptr<i64>(), G.F, G.Cg(), a.kh, a.kw, p, conv_dilated(a));
            a.wg[j] = upload(wg.data(), wg.size());
        }
        if (a.nbands > 0 && p <= 255) {
            // [F16][kh][kw][Cpad] centered int8 (im2col order ci*kh*kw + dy*kw + dx -> (dy, dx, ci))
            const std::vector<int8_t> w8r = conv_w8r(a, w8, static_cast<int>(G.F));
            a.w8r[j] = upload(w8r.data(), w8r.size());
        } else {
            a.w8r[j] = nullptr;
        }
        a.zc[j] = upload(zc.data(), zc.size());
        a.bias[j] = hard_ ? zero_i16(static_cast<size_t>(B_) * G.F * nr_comps(p))
                          : upload_i16_rows(li, arr_name("bias.", j, ""));
    }
    set_label_rows(a);
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const int B = B_;
    add_op(lname, [a, x, y, B](hipStream_t st) { launch_conv(a, x, y, B, st); });
    set_out(w, g, G.out_size(), w.nxt());
}

// Transposed conv: its stride-1 sub-pixel view (layers.h ConvTGeom) through the dense conv's plan and kernels,
// whose epilogue scatters the view's F sh sw filters to the output (ConvArgs::tsc). Hardened encoding only: the
// evaluator computes the bare sum, so the zero counts and the bias rows are all zero.
void HipEvaluator::plan_convt(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    DASH_CHECK(hard_, "conv_transpose2d exists in the hardened encoding only");
    ConvTGeom G(g);
    DASH_CHECK(G.C * G.H * G.W == w.N, "conv_transpose2d input size mismatch");
    ConvArgs a{};
    a.crt = w.crt;
    convt_view_args(a, static_cast<int>(G.C), static_cast<int>(G.H), static_cast<int>(G.W), static_cast<int>(G.F),
                    static_cast<int>(G.kh), static_cast<int>(G.kw), static_cast<int>(G.sh), static_cast<int>(G.sw),
                    static_cast<int>(G.ph), static_cast<int>(G.pw), static_cast<int>(G.OH), static_cast<int>(G.OW));
    a.use_mfma = mfma_ ? 1 : 0;
    conv_layer_plan(a, mfma_ && conv_img_enabled());
    a.img_off[0] = 0;
    for (int j = 0; j < k_; ++j) a.img_off[j + 1] = a.img_off[j] + static_cast<i64>(B_) * w.crt.n[j];
    const Array& wt = g.arr("w");
    DASH_CHECK(static_cast<i64>(wt.count()) == G.F * G.K(), "conv_transpose2d weight shape");
    const std::vector<i64> wv = G.view_weights(wt.ptr<i64>());
    const i64 VF = G.VF(), K = G.VK();
    const std::vector<int32_t> zc(static_cast<size_t>(VF), 0);
    const int32_t* dzc = upload(zc.data(), zc.size());
    for (int j = 0; j < k_; ++j) {
        const int p = crt_[j];
        std::vector<int16_t> wm(static_cast<size_t>(VF * K));
        std::vector<int8_t> w8(static_cast<size_t>(VF) * a.Kpad, 0);
        for (i64 f = 0; f < VF; ++f)
            for (i64 q = 0; q < K; ++q) {
                const int v = static_cast<int>(wv[static_cast<size_t>(f * K + q)] % p);
                wm[static_cast<size_t>(f * K + q)] = static_cast<int16_t>(v);
                w8[static_cast<size_t>(f) * a.Kpad + q] = static_cast<int8_t>(v > p / 2 ? v - p : v);
            }
        a.w[j] = upload(wm.data(), wm.size());
        a.w8[j] = (mfma_ && p <= 255) ? upload(w8.data(), w8.size()) : nullptr;
        a.wg[j] = nullptr;
        a.w8r[j] = nullptr;
        if (a.nbands > 0 && p <= 255) {
            const std::vector<int8_t> w8r = conv_w8r(a, w8, static_cast<int>(VF));
            a.w8r[j] = upload(w8r.data(), w8r.size());
        }
        a.zc[j] = dzc;
        a.bias[j] = zero_i16(static_cast<size_t>(B_) * VF * nr_comps(p));
    }
    set_label_rows(a);
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const int B = B_;
    add_op(lname, [a, x, y, B](hipStream_t st) { launch_conv(a, x, y, B, st); });
    set_out(w, g, G.out_size(), w.nxt());
}

// Nearest-neighbour upsampling: a label gather (free: no tables), any moduli
void HipEvaluator::plan_upsample(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    UpGeom G(g.p);
    DASH_CHECK(G.C * G.H * G.W == w.N, "upsample input size mismatch");
    const i64 No = G.out_size(), NN = w.N;
    std::vector<i64> idx(static_cast<size_t>(No));
    for (i64 o = 0; o < No; ++o) idx[static_cast<size_t>(o)] = G.src(o);
    const int64_t* didx = upload(idx.data(), idx.size());
    const CrtInfo ci = crt_info(w.mods);
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const int B = B_;
    add_op(lname, [x, NN, y, No, didx, ci, B](hipStream_t st) { launch_copy_gather(x, NN, y, No, didx, ci, B, st); });
    set_out(w, g, No, w.nxt());
}

// Gather: the labels moved by a public index map (free: no tables), any moduli. A layer with in_src reads the
// saved copy of that output where it lies, as plan_mul reads its operand; N and the moduli come from the slot.
// The form rule: the dword kernel where Nout % 4 == 0 and every base pointer is 4-byte aligned, else the byte
// kernel; DASH_GATHER_FORM=byte forces the byte form (A/B runs).
void HipEvaluator::plan_gather(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    Act x = act_of(w.cur), y = act_of(w.nxt());
    if (g.p.count("in_src")) {
        const i64 src = g.param("in_src");
        DASH_CHECK(src >= -1 && src + 1 < static_cast<i64>(saved_.size()) && !saved_[src + 1].empty(),
                   "in_src source not saved");
        w.N = w.saved_n[src + 1];
        w.mods = w.saved_mods[src + 1];
        for (int j = 0; j < k_; ++j) x.p[j] = saved_[src + 1][j];
    }
    const GatherGeom G(g.p, w.N);
    const i64 No = G.out_size(), NN = w.N;
    bool dword = No % 4 == 0;
    for (int j = 0; j < k_; ++j)
        dword = dword && reinterpret_cast<uintptr_t>(x.p[j]) % 4 == 0 && reinterpret_cast<uintptr_t>(y.p[j]) % 4 == 0;
    if (const char* f = std::getenv("DASH_GATHER_FORM"))
        if (std::string(f) == "byte") dword = false;
    const int32_t* d4 = nullptr;
    const int64_t* d8 = nullptr;
    if (dword) {
        std::vector<int32_t> i4(static_cast<size_t>((No + 3) / 4 * 4), 0);
        for (i64 o = 0; o < No; ++o) i4[static_cast<size_t>(o)] = static_cast<int32_t>(G.src(o));
        d4 = upload(i4.data(), i4.size());
    } else {
        d8 = upload(G.idx->data(), G.idx->size());
    }
    const CrtInfo ci = crt_info(w.mods);
    const int B = B_;
    add_op(lname, [x, NN, y, No, d4, d8, ci, B](hipStream_t st) { launch_gather(x, NN, y, No, d4, d8, ci, B, st); });
    set_out(w, g, No, w.nxt());
}

// Bilinear: the separable two-tap label stencil with public weights (free: no tables), any moduli of at most
// kActMaxModulus. The form rule: the dword kernel where OW % 4 == 0 and every base pointer is 4-byte aligned, else
// the byte kernel; DASH_BILINEAR_FORM=byte forces the byte form (A/B runs).
void HipEvaluator::plan_bilinear(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    DASH_CHECK(hard_, "bilinear exists in the hardened encoding only");
    const BilinearGeom G(g.p);
    DASH_CHECK(G.in_size() == w.N, "bilinear input size mismatch");
    for (int p : w.mods) DASH_CHECK(p <= kActMaxModulus, "bilinear: residue modulus above 255");
    Act x = act_of(w.cur), y = act_of(w.nxt());
    bool dword = G.OW % 4 == 0;
    for (int j = 0; j < k_; ++j) dword = dword && reinterpret_cast<uintptr_t>(y.p[j]) % 4 == 0;
    if (const char* f = std::getenv("DASH_BILINEAR_FORM"))
        if (std::string(f) == "byte") dword = false;
    BilinearArgs a{};
    const BilinearTables t = bilinear_tables(a, G, w.mods.data(), static_cast<int>(w.mods.size()));
    a.rows = upload(t.rows.data(), t.rows.size());
    a.cols = upload(t.cols.data(), t.cols.size());
    a.wrow = upload(t.wrow.data(), t.wrow.size());
    a.wcol = upload(t.wcol.data(), t.wcol.size());
    const CrtInfo ci = crt_info(w.mods);
    const int B = B_;
    add_op(lname, [a, dword, x, y, ci, B](hipStream_t st) { launch_bilinear(a, dword, x, y, ci, B, st); });
    set_out(w, g, G.out_size(), w.nxt());
}

void HipEvaluator::plan_relu(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const Env e = w.env;
    const i64 smode = g.param("smode", 0);
    Act x = act_of(w.cur), y = act_of(w.nxt());
    if (smode == 2) {  // sign from the preceding rescale (RescaleMrsPlan::sign_last)
        DASH_CHECK(li > 0 && m0.layers[li - 1].kind == K_RESCALE && m0.layers[li - 1].param("sign_out", 0) == 1,
                   "joint ReLU must follow a sign-producing rescale");
        const SignArgs sa = joint_sign_args(w, li, w.N);
        const u128* gt = upload_tables(li, "mm.g");
        const u128* et = upload_tables(li, "mm.e");
        if (w.pending == Walk::Pending::relu) {
            const MrsArgs ma = w.pending_a;
            w.pending = Walk::Pending::none;
            add_op(lname + ".C", [ma, sa, x, y, gt, et, e](hipStream_t st) {
                launch_rescale_relu_out(ma, sa, x, y, gt, et, e.B, e.mc, e.ag, st);
            });
        } else {
            add_op(lname + ".C", [sa, x, y, gt, et, e](hipStream_t st) {
                launch_relu_joint(sa, x, y, gt, et, e.B, e.mc, e.ag, st);
            });
        }
    } else if (smode == 1) {  // exact mixed-radix sign (gadgets.h SignMrsPlan)
        DASH_CHECK(hard_, "the mixed-radix sign exists in the hardened encoding only");
        const MrsArgs a = mrs_sign_args(w, li, "mrs", w.N, gate_base(li + 1, 1), gate_base(li + 1, 2), ny_, nullptr);
        const SignArgs sa = joint_sign_args(w, li, w.N);
        const u128* gt = upload_tables(li, "mm.g");
        const u128* et = upload_tables(li, "mm.e");
        add_op(lname + ".mrs", [a, sa, x, y, gt, et, e](hipStream_t st) {
            launch_relu_mrs(a, sa, x, y, gt, et, e.B, e.mc, e.ag, st);
        });
    } else {
        SignPlan sp(crt_, m0.h.mrs, {2}, 0, 1, m0.h.sign_fused != 0);
        const Sign s = make_sign(li, "", sp, w.N, 1, gate_base(li + 1, 1), gate_base(li + 1, 2));
        const SignArgs a = s.a;
        const int maxn = s.maxn;
        const u128* gt = upload_tables(li, "mm.g");
        const u128* et = upload_tables(li, "mm.e");
        add_op(lname + ".A", [a, x, e](hipStream_t st) { launch_sign_approx(a, x, e.mc, e.ag, st); });
        add_op(lname + ".B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
        add_op(lname + ".C", [a, x, y, gt, et, e](hipStream_t st) { launch_relu_mult(a, x, y, gt, et, e.mc, st); });
    }
    set_out(w, g, w.N, w.nxt());
}

// gadgets.h LeakyPlan: plan_relu's ops for the layer's resolved sign construction with the leaky multiply in the
// ReLU multiply's place; the layer's factor table [channel][residue] is public and uploaded once
void HipEvaluator::plan_leaky(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const Env e = w.env;
    const i64 smode = g.param("smode", 0);
    DASH_CHECK(w.mods == crt_, "leaky_relu: the input is not on the CRT base");
    DASH_CHECK(w.N < (i64{1} << 32), "leaky_relu: more than 2^32 elements");
    const LeakyPlan lp(g.param("s"), g.vec("n"), g.param("bc"), w.N);
    const std::vector<uint16_t> tab = lp.table(crt_);
    LeakyTab lk{upload(tab.data(), tab.size()), static_cast<uint32_t>(lp.n.size() == 1 ? w.N : lp.bc)};
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const u128* gt = upload_tables(li, "mm.g");
    const u128* et = upload_tables(li, "mm.e");
    if (smode == 2) {
        DASH_CHECK(li > 0 && m0.layers[li - 1].kind == K_RESCALE && m0.layers[li - 1].param("sign_out", 0) == 1,
                   "joint LeakyRelu must follow a sign-producing rescale");
        const SignArgs sa = joint_sign_args(w, li, w.N);
        if (w.pending == Walk::Pending::leaky) {
            const MrsArgs ma = w.pending_a;
            w.pending = Walk::Pending::none;
            add_op(lname + ".C", [ma, sa, lk, x, y, gt, et, e](hipStream_t st) {
                launch_rescale_leaky_out(ma, sa, lk, x, y, gt, et, e.B, e.mc, e.ag, st);
            });
        } else {
            add_op(lname + ".C", [sa, lk, x, y, gt, et, e](hipStream_t st) {
                launch_leaky_mult(sa, lk, x, y, gt, et, e.mc, st);
            });
        }
    } else if (smode == 1) {
        DASH_CHECK(hard_, "the mixed-radix sign exists in the hardened encoding only");
        const MrsArgs a = mrs_sign_args(w, li, "mrs", w.N, gate_base(li + 1, 1), gate_base(li + 1, 2), ny_, nullptr);
        const SignArgs sa = joint_sign_args(w, li, w.N);
        add_op(lname + ".mrs", [a, sa, lk, x, y, gt, et, e](hipStream_t st) {
            launch_leaky_mrs(a, sa, lk, x, y, gt, et, e.B, e.mc, e.ag, st);
        });
    } else {
        SignPlan sp(crt_, m0.h.mrs, {2}, 0, 1, m0.h.sign_fused != 0);
        const Sign s = make_sign(li, "", sp, w.N, 1, gate_base(li + 1, 1), gate_base(li + 1, 2));
        const SignArgs a = s.a;
        const int maxn = s.maxn;
        add_op(lname + ".A", [a, x, e](hipStream_t st) { launch_sign_approx(a, x, e.mc, e.ag, st); });
        add_op(lname + ".B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
        add_op(lname + ".C", [a, lk, x, y, gt, et, e](hipStream_t st) { launch_leaky_mult(a, lk, x, y, gt, et, e.mc, st); });
    }
    set_out(w, g, w.N, w.nxt());
}

// gadgets.h PwlPlan: the compressed labels of x, one sign evaluation per kept breakpoint on the same labels (each
// with its own tables and gate, into its own key buffer), then one multiply pass that applies every breakpoint's
// half gates and the linear combination
void HipEvaluator::plan_pwl(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    DASH_CHECK(hard_, "the PiecewiseLinear layer exists in the hardened encoding only");
    DASH_CHECK(w.mods == crt_, "pwl: the input is not on the CRT base");
    const PwlPlan pp(crt_, g.param("s"), g.vec("T"), g.vec("A"), g.param("V"));
    for (int p : crt_) DASH_CHECK(p <= 255, "pwl: the factor table holds bytes");
    ensure_kpwl(w);
    const std::vector<uint8_t> fac = pp.table();
    PwlArgs pa{};
    pa.crt = w.crt;
    pa.N = w.N;
    pa.m = pp.m();
    pa.kx = hx_;
    pa.colx = colx_;
    pa.fac = upload(fac.data(), fac.size());
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const Env e = w.env;
    const bool exact = g.param("smode", 0) == 1;
    {
        u128* kx = hx_;
        uint16_t* colx = colx_;
        add_op(lname + ".K", [pa, kx, colx, x, e](hipStream_t st) { launch_pwl_key(pa, kx, colx, x, e.B, e.mc, st); });
    }
    for (int i = 0; i < pp.m(); ++i) {
        const std::string pre = PwlPlan::prefix_of(i);
        const uint64_t sgate = gate_base(li + 1, PwlPlan::sign_slot(i));
        pa.mgate0[i] = gate_base(li + 1, PwlPlan::mult_slot(i));
        pa.key[i] = kpwl_[i];
        pa.gtab[i] = upload_tables(li, pre + "mm.g");
        pa.etab[i] = upload_tables(li, pre + "mm.e");
        if (exact) {  // the label itself kept, no y-row pads: the multiply derives them (as a Clip's)
            const MrsArgs a = mrs_sign_args(w, li, pre + "mrs", w.N, sgate, pa.mgate0[i], 0, kpwl_[i]);
            add_op(lname + "." + pre + "mrs", [a, x, e](hipStream_t st) {
                launch_clip_sign_mrs(a, x, e.B, e.mc, e.ag, st);
            });
        } else {
            SignPlan sp(crt_, m0.h.mrs, {2}, 0, 1, m0.h.sign_fused != 0);
            const Sign s = make_sign(li, pre, sp, w.N, 0, sgate, 0);
            SignArgs a = s.a;
            a.outP = kpwl_[i];  // nout = 1: [B][N]
            const int maxn = s.maxn;
            add_op(lname + "." + pre + "A", [a, x, e](hipStream_t st) { launch_sign_approx(a, x, e.mc, e.ag, st); });
            add_op(lname + "." + pre + "B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
        }
    }
    add_op(lname + ".C", [pa, x, y, e](hipStream_t st) { launch_pwl_mult(pa, x, y, e.B, e.mc, st); });
    set_out(w, g, w.N, w.nxt());
}

// gadgets.h ClipPlan: the half gates' keys of x, the sign evaluation once per bound on the same labels (each into
// its own scratch), then the multiply + cap
void HipEvaluator::plan_clip(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    DASH_CHECK(hard_, "the Clip layer exists in the hardened encoding only");
    ensure_ks(w, 2);
    ClipArgs ca{};
    ca.crt = w.crt;
    ca.N = w.N;
    ca.hx = hx_;
    ca.colx = colx_;
    ca.klo = ks_[0];
    ca.khi = ks_[1];
    ca.gtab = upload_tables(li, "mm.g");
    ca.etab = upload_tables(li, "mm.e");
    ca.cap = upload_tables(li, "cap");
    ca.mgate0 = gate_base(li + 1, 2);
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const Env e = w.env;
    const i64 smode = g.param("smode", 0);
    if (smode == 2) {
        // joint variant: the rescale before it left both sign labels (ks_) and the half-gate keys of its output
        // (hx_ / colx_); only the multiply + cap is left
        DASH_CHECK(li > 0 && m0.layers[li - 1].kind == K_RESCALE && m0.layers[li - 1].param("sign_out", 0) == 1 &&
                       !g.p.count("in_src") && g.vec("lo").at(0) == 0,
                   "joint Clip must follow a sign-producing rescale");
        if (w.pending == Walk::Pending::clip) {
            const MrsArgs ma = w.pending_a;
            w.pending = Walk::Pending::none;
            add_op(lname + ".C", [ma, ca, x, y, e](hipStream_t st) {
                launch_rescale_clip_out(ma, ca, x, y, e.B, e.mc, e.ag, st);
            });
        } else {
            add_op(lname + ".C", [ca, x, y, e](hipStream_t st) { launch_clip_mult(ca, x, y, e.B, e.mc, st); });
        }
        set_out(w, g, w.N, w.nxt());
        return;
    }
    const bool exact = smode == 1;
    // the half gates' keys of x: the approximate sign's first phase compresses x anyway and writes them (lower
    // bound's run, below); the mixed-radix chain does not, so they get a pass of their own
    if (exact) {
        u128* hx = hx_;
        uint16_t* colx = colx_;
        add_op(lname + ".H", [ca, hx, colx, x, e](hipStream_t st) {
            launch_clip_hash(ca, hx, colx, x, e.B, e.mc, e.ag, st);
        });
    }
    for (int side = 0; side < 2; ++side) {
        const std::string pre = side ? "hi." : "lo.";
        const uint64_t sgate = gate_base(li + 1, side ? 3 : 1);
        if (exact) {  // exact mixed-radix sign, label kept in ks; no y-row pads: the multiply forms the pads of
                      // u = s_lo + s_hi itself
            const MrsArgs a = mrs_sign_args(w, li, pre + "mrs", w.N, sgate, ca.mgate0, 0, ks_[side]);
            add_op(lname + "." + pre + "mrs", [a, x, e](hipStream_t st) {
                launch_clip_sign_mrs(a, x, e.B, e.mc, e.ag, st);
            });
        } else {
            SignPlan sp(crt_, m0.h.mrs, {2}, 0, 1, m0.h.sign_fused != 0);
            const Sign s = make_sign(li, pre, sp, w.N, 0, sgate, 0);
            SignArgs a = s.a;
            a.outP = ks_[side];  // nout = 1: [B][N]
            if (side == 0) {  // (TW_MMG, j) pads of x_j under the multiply's gate, as a ReLU's phase A
                a.hx = hx_;
                a.colx = colx_;
                a.mgate0 = ca.mgate0;
            }
            const int maxn = s.maxn;
            add_op(lname + "." + pre + "A", [a, x, e](hipStream_t st) { launch_sign_approx(a, x, e.mc, e.ag, st); });
            add_op(lname + "." + pre + "B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
        }
    }
    add_op(lname + ".C", [ca, x, y, e](hipStream_t st) { launch_clip_mult(ca, x, y, e.B, e.mc, st); });
    set_out(w, g, w.N, w.nxt());
}

void HipEvaluator::plan_sign(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    SignPlan sp(crt_, m0.h.mrs, crt_, -1, 1, m0.h.sign_fused != 0);
    const Sign s = make_sign(li, "", sp, w.N, 0, gate_base(li + 1, 1), 0);
    const SignArgs a = s.a;
    const int maxn = s.maxn;
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const Env e = w.env;
    const CrtInfo crt = w.crt;
    const u128* outP = outP_;
    const i64 NN = w.N;
    add_op(lname + ".A", [a, x, e](hipStream_t st) { launch_sign_approx(a, x, e.mc, e.ag, st); });
    add_op(lname + ".B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
    add_op(lname + ".unpack", [outP, y, crt, NN, e](hipStream_t st) { launch_unpack(outP, crt.k, y, crt, e.mc, NN, e.B, st); });
    set_out(w, g, w.N, w.nxt());
}

// every rescale works in place, on the current buffer
void HipEvaluator::plan_rescale(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const i64 mode = g.param("mode", 0);
    const i64 iters = g.param("iters");
    if (mode == 2)
        plan_rescale_mrs(w, li, g, lname);
    else if (mode == 0)
        plan_rescale_legacy(w, li, iters, act_of(w.cur), lname);
    else
        plan_rescale_redash(w, li, g, lname);
    set_out(w, g, w.N, w.cur);
}

// mixed-radix construction of the legacy function (gadgets.h RescaleMrsPlan)
void HipEvaluator::plan_rescale_mrs(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const i64 N = w.N;
    const bool so = g.param("sign_out", 0) == 1;  // joint: the next ReLU's sign -> hs_, cs_
    const RescaleMrsPlan P(crt_, static_cast<int>(g.param("l")), so);
    DASH_CHECK(P.T <= m0.h.max_mod, "model lacks the mod-2^(l+1) label constants");
    MrsArgs a{};
    a.crt = w.crt;
    a.T = static_cast<int>(P.T);
    a.N = N;
    a.n_tab = P.n_tab;
    a.tab = upload_tables(li, "mrs");
    for (int i = 0; i < k_; ++i) {
        a.dig_off[i] = P.dig_off[i];
        a.sinv[i] = static_cast<int>(P.Sinv[i]);
    }
    a.fin_off = P.fin_off;
    const int bits = P.l + 1, nf = nr_comps(static_cast<int>(P.T));
    a.hmask = 0;
    for (int f = 0; f < nf; ++f) a.hmask |= static_cast<u128>(1) << (bits * f + bits - 1);
    a.pf = outP_;  // [B][k][N] <= the sign outputs' scratch
    ensure_mrs_ps(w);
    a.ps = mrs_ps_;
    a.mode = so ? 2 : 0;
    a.hs = hs_;
    a.cs = cs_;
    a.hx = hx_;
    a.colx = colx_;
    DASH_CHECK(hard_, "the mixed-radix rescale exists in the hardened encoding only");
    a.gate0 = gate_base(li + 1, 30);
    a.rgate0 = so ? gate_base(li + 2, 2) : 0;  // the joint ReLU (next layer)'s half gates
    a.ny = ny_;
    a.ys = ys_;
    const bool has_next = li + 1 < m0.layers.size();
    if (so && has_next && m0.layers[li + 1].kind == K_CLIP && m0.layers[li + 1].param("smode", 0) == 2) {
        plan_rescale_clip(w, li, a, lname);
        return;
    }
    // joint ReLU next and this output not kept for a later layer: the ReLU's op can write both outputs in one
    // pass (launch_rescale_relu_out), here only the chain runs. The rescaled label is then never written: the
    // fused kernels keep it in LDS. Which launches take it is launch.h joint_fuse: batches of at most 2 GCs
    // (latency_b1 2.21 -> 2.14 ms), and staged shapes from 13,824 elements over the batch, where the throughput
    // form wins on every MiniONN layer (24-GC step 9.08 -> 7.55 ms, profiles/ab/joint_fused/README.md);
    // hip_set_joint_fuse (initially DASH_JOINT_FUSE=0/1) forces it off/on.
    const bool defer = dev::joint_fuse(N, B_) && so && has_next && m0.layers[li + 1].kind == K_RELU &&
                       m0.layers[li + 1].param("smode", 0) == 2 && !w.keep[li + 1] &&
                       !m0.layers[li + 1].p.count("in_src");
    // a joint LeakyRelu next: the same deferral where the throughput form runs (launch.h leaky_fuse); the
    // small-batch fused forms have no leaky counterpart, so those launches keep the output-hash kernel here
    const bool defer_leaky = dev::leaky_fuse(N, B_) && so && has_next && m0.layers[li + 1].kind == K_LEAKY &&
                             m0.layers[li + 1].param("smode", 0) == 2 && !w.keep[li + 1] &&
                             !m0.layers[li + 1].p.count("in_src");
    if (defer || defer_leaky) {
        w.pending_a = a;
        w.pending = defer ? Walk::Pending::relu : Walk::Pending::leaky;
    }
    Act x = act_of(w.cur);
    const Env e = w.env;
    const bool dfr = defer || defer_leaky;
    add_op(lname + ".mrs", [a, x, e, dfr](hipStream_t st) { launch_rescale_mrs(a, x, e.B, e.mc, e.ag, st, dfr); });
}

// A joint Clip next (gadgets.h ClipPlan, joint variant): the chain keeps its mod-2 key as the Clip's lower sign
// label (ks_[0], no y-row pads), the Clip's upper sign chain (mode 1, the Clip layer's tables and slot-3 gate) runs
// on the same input labels into ks_[1], and only then the output kernel rewrites x in place, leaving y's half-gate
// keys under the Clip's multiply gate in hx_ / colx_. Both chains share mrs_ps_; the mode-1 chain writes neither
// a.pf nor outP_, so the rescale's final payloads wait there.
void HipEvaluator::plan_rescale_clip(Walk& w, size_t li, MrsArgs a, const std::string& lname) {
    const GLayer& gc = tmpl_->layers[li + 1];
    const i64 N = w.N;
    DASH_CHECK(!gc.p.count("in_src"), "joint Clip must read the rescale before it");
    ensure_ks(w, 2);
    a.ks = ks_[0];
    a.ny = 0;
    DASH_CHECK(gc.arr("hi.mrs").shape[0] == N && gc.arr("hi.mrs").shape[1] == std::max<i64>(SignMrsPlan(crt_).n_tab, 1),
               "joint Clip upper sign table shape");
    const MrsArgs h = mrs_sign_args(w, li + 1, "hi.mrs", N, gate_base(li + 2, 3), a.rgate0, 0, ks_[1]);
    Act x = act_of(w.cur);
    const Env e = w.env;
    add_op(lname + ".mrs", [a, x, e](hipStream_t st) { launch_rescale_mrs(a, x, e.B, e.mc, e.ag, st, true); });
    // streamed tables: the Clip layer's window was issued by this layer's stage op
    if (stream_)
        add_op(lname + ".wait", [this, li](hipStream_t st) {
            HIPCHECK(hipStreamWaitEvent(st, ready_[li + 1], 0));
        });
    add_op(lname + ".clip_hi", [h, x, e](hipStream_t st) { launch_clip_sign_mrs(h, x, e.B, e.mc, e.ag, st); });
    // output not kept for a later layer and the fusion on (launch.h clip_fuse): the Clip's op writes both outputs
    // in one pass (launch_rescale_clip_out), the rescaled label stays in LDS
    if (dev::clip_fuse(N, B_) && !w.keep[li + 1]) {
        w.pending_a = a;
        w.pending = Walk::Pending::clip;
    } else {
        add_op(lname + ".out", [a, x, e](hipStream_t st) { launch_rescale_mrs_out(a, x, e.B, e.mc, e.ag, st); });
    }
}

// ReDash rescale: per iteration and factor the factor residue's hash and the update, then the base extension
// that restores the factor residues and the downshift. (The sign base extension in place of the BEPlan exists in
// the legacy mode only: plan_rescale_legacy.)
void HipEvaluator::plan_rescale_redash(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const i64 N = w.N, iters = g.param("iters");
    const CrtInfo crt = w.crt;
    const Env e = w.env;
    Act x = act_of(w.cur);
    std::vector<int> factors;
    for (auto v : g.vec("s")) factors.push_back(static_cast<int>(v));
    const RescalePlan P(crt_, m0.h.mrs, factors, false, m0.h.sign_fused != 0);
    for (i64 it = 0; it < iters; ++it) {
        const std::string pre = arr_name("it", static_cast<int>(it), ".");
        const u128* trans = upload_tables(li, pre + "trans");
        i64 off = 0;
        for (size_t f = 0; f < P.factors.size(); ++f) {
            const int fi = P.factor_idx[f], s = P.factors[f];
            const int add_up = f == 0 ? 1 : 0;
            const int16_t* up = up_rows_ + lab_off_[fi];
            u128* h0 = h0_;
            uint16_t* col0 = col0_;
            const int ls = lab_stride_;
            const int hd = hard_ ? 1 : 0;
            add_op(lname + ".hash", [x, fi, s, up, ls, add_up, N, h0, col0, e, hd](hipStream_t st) {
                launch_rescale_hash(x, fi, s, up, ls, add_up, N, e.B, h0, col0, e.mc, e.ag, st, hd);
            });
            RescaleArgs ra{};
            ra.crt = crt;
            ra.N = N;
            ra.fi = fi;
            ra.s = s;
            ra.add_up = add_up;
            set_active(ra, P, f, trans);
            ra.off = off;
            off += static_cast<i64>(P.active[f].size()) * s;
            ra.up = up_rows_;
            set_label_rows(ra);
            ra.hard = hd;
            ra.gate0 = gate_base(li + 1, 10 + it);
            ra.factor = static_cast<int>(f);
            add_op(lname + ".update", [ra, x, e](hipStream_t st) { launch_rescale_update(ra, x, e.B, e.mc, st); });
        }
        const BEArgs ba = be_args(w, P.be, li, pre + "be", N, gate_base(li + 1, 10 + it));
        add_op(lname + ".be", [ba, x, e](hipStream_t st) { launch_base_ext(ba, x, e.B, e.mc, e.ag, st); });
        const int16_t* down = upload_const_rows(
            [&](int j) { return "down." + std::to_string(P.sprod) + "." + std::to_string(j); });
        const u128* signP = nullptr;  // no sign base extension: the base extension above restored the residues
        const int ls = lab_stride_;
        const int* loff = d_lab_off_;
        add_op(lname + ".post", [x, crt, N, signP, down, ls, loff, e](hipStream_t st) {
            launch_rescale_post(x, crt, N, e.B, signP, down, ls, loff, e.mc, st);
        });
    }
}

void HipEvaluator::plan_rescale_legacy(Walk& w, size_t li, i64 iters, Act x, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const i64 N = w.N;
    const CrtInfo crt = w.crt;
    const Env e = w.env;
    const int ls = lab_stride_;
    DASH_CHECK(crt_[0] == 2, "legacy rescale needs crt[0] == 2");
    // per-GC constants: delta = up - down (all residues), du = bits(up0) ^ bits(down0)
    const int16_t* delta = nullptr;
    const u128* du = nullptr;
    {
        int16_t* dd = dalloc<int16_t>(static_cast<size_t>(B_) * lab_stride_);
        u128* ddu = dalloc<u128>(B_);
        const int k = k_;
        std::vector<int> off(lab_off_, lab_off_ + k_), crtv = crt_;
        add_small(reinterpret_cast<uint8_t*>(dd), sizeof(int16_t) * ls, sizeof(int16_t) * ls,
                  [ls, k, off, crtv](const GarbledModel& m, uint8_t* hb) {
            int16_t* h = reinterpret_cast<int16_t*>(hb);
            std::fill(h, h + ls, int16_t(0));
            for (int j = 0; j < k; ++j) {
                const int p = crtv[j], n = nr_comps(p);
                const int16_t* up = m.consts.at("up." + std::to_string(j)).ptr<int16_t>();
                const int16_t* dn = m.consts.at("down.2." + std::to_string(j)).ptr<int16_t>();
                for (int c = 0; c < n; ++c) h[off[j] + c] = static_cast<int16_t>(pmod(up[c] - dn[c], p));
            }
        });
        add_small(reinterpret_cast<uint8_t*>(ddu), sizeof(u128), sizeof(u128), [](const GarbledModel& m, uint8_t* hb) {
            u128 pk = 0;
            const int n = nr_comps(2);
            const int16_t* up = m.consts.at("up.0").ptr<int16_t>();
            const int16_t* dn = m.consts.at("down.2.0").ptr<int16_t>();
            for (int c = 0; c < n; ++c) pk |= static_cast<u128>((up[c] ^ dn[c]) & 1) << c;
            std::memcpy(hb, &pk, sizeof(u128));
        });
        delta = dd;
        du = ddu;
    }
    const int16_t* down = upload_const_rows([&](int j) { return "down.2." + std::to_string(j); });
    const RescalePlan P(crt_, m0.h.mrs, {2}, true, m0.h.sign_fused != 0);
    for (i64 it = 0; it < iters; ++it) {
        const std::string pre = arr_name("it", static_cast<int>(it), ".");
        const u128* trans = upload_tables(li, pre + "trans");
        const Sign sg = make_sign(li, pre, P.sign, N, 0);
        const SignArgs sa = sg.a;
        const int maxn = sg.maxn;
        u128* h0 = h0_;
        uint16_t* col0 = col0_;
        if (it == 0) {
            const int16_t* up = up_rows_ + lab_off_[0];
            add_op(lname + ".hash", [x, up, ls, N, h0, col0, e](hipStream_t st) {
                launch_rescale_hash(x, 0, 2, up, ls, 1, N, e.B, h0, col0, e.mc, e.ag, st);
            });
        } else {
            const u128* sp = outP_;
            add_op(lname + ".hash", [sp, du, N, h0, col0, e](hipStream_t st) {
                launch_rescale_hash_sign(sp, du, N, e.B, h0, col0, e.ag, st);
            });
        }
        RescaleArgs ra{};
        ra.crt = crt;
        ra.N = N;
        ra.fi = 0;
        ra.s = 2;
        ra.add_up = 1;
        set_active(ra, P, 0, trans);
        ra.off = 0;
        set_label_rows(ra);
        const int16_t* dl = it == 0 ? up_rows_ : delta;
        const u128* zh = zh_;
        add_op(lname + ".upd+A", [ra, sa, x, dl, zh, e](hipStream_t st) {
            launch_rescale_update_approx(ra, sa, x, dl, zh, e.B, e.mc, e.ag, st);
        });
        add_op(lname + ".B", [sa, maxn, e](hipStream_t st) { launch_sign_chain(sa, maxn, e.mc, e.ag, st); });
    }
    const u128* signP = outP_;
    const int* loff = d_lab_off_;
    add_op(lname + ".post", [x, crt, N, signP, down, ls, loff, e](hipStream_t st) {
        launch_rescale_post(x, crt, N, e.B, signP, down, ls, loff, e.mc, st);
    });
}

// K_MAXPOOL and K_MAX: a gather of the windows, then one ReLU of pairwise differences per level of the max tree
void HipEvaluator::plan_max(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const GarbledModel& m0 = *tmpl_;
    const CrtInfo crt = w.crt;
    const Env e = w.env;
    const int B = B_;
    const i64 NN = w.N;
    const int cur = w.cur, nxt = w.nxt();
    i64 Nout, K;
    std::vector<i64> idx;
    if (g.kind == K_MAXPOOL) {
        PoolGeom G(g.p);
        Nout = G.out_size();
        K = G.kh * G.kw;
        std::vector<i64> win;
        for (i64 o = 0; o < Nout; ++o) {
            G.window(o, win);
            idx.insert(idx.end(), win.begin(), win.end());
        }
    } else {
        Nout = 1;
        K = NN;
        for (i64 i = 0; i < NN; ++i) idx.push_back(i);
    }
    const int64_t* didx = upload(idx.data(), idx.size());
    MaxTree T(K);
    SignPlan sp(crt_, m0.h.mrs, {2}, 0, 1, m0.h.sign_fused != 0);
    // buffers: the candidate values ping-pong between bufs 2 / 3; the differences reuse buffer `cur` (its content
    // is no longer needed) and the ReLU's output goes to `nxt`
    int va = 2, vb = 3;
    Act xin = act_of(cur), v0 = act_of(va);
    add_op(lname + ".gather", [xin, NN, v0, Nout, K, didx, crt, B](hipStream_t st) {
        launch_copy_gather(xin, NN, v0, Nout * K, didx, crt, B, st);
    });
    for (size_t lv = 0; lv < T.ops.size(); ++lv) {
        const int ops = T.ops[lv], cnt = T.cnt[lv], cnt1 = T.cnt[lv + 1];
        const std::string pre = arr_name("lv", static_cast<int>(lv), ".");
        const Sign s = make_sign(li, pre, sp, Nout * ops, 1, gate_base(li + 1, 20 + 2 * lv), gate_base(li + 1, 21 + 2 * lv));
        const SignArgs a = s.a;
        const int maxn = s.maxn;
        const u128* gt = upload_tables(li, pre + "mm.g");
        const u128* et = upload_tables(li, pre + "mm.e");
        Act V = act_of(va), D = act_of(cur), Rr = act_of(nxt), NV = act_of(vb);
        const i64 Nv = Nout * cnt;
        add_op(lname + ".diff", [V, Nv, D, Nout, ops, cnt, crt, B](hipStream_t st) {
            launch_pair_diff(V, Nv, D, Nout, ops, cnt, crt, B, st);
        });
        add_op(lname + ".A", [a, D, e](hipStream_t st) { launch_sign_approx(a, D, e.mc, e.ag, st); });
        add_op(lname + ".B", [a, maxn, e](hipStream_t st) { launch_sign_chain(a, maxn, e.mc, e.ag, st); });
        add_op(lname + ".C", [a, D, Rr, gt, et, e](hipStream_t st) { launch_relu_mult(a, D, Rr, gt, et, e.mc, st); });
        add_op(lname + ".add", [V, Nv, Rr, NV, Nout, ops, cnt, cnt1, crt, B](hipStream_t st) {
            launch_pair_add(V, Nv, Rr, NV, Nout, ops, cnt, cnt1, crt, B, st);
        });
        std::swap(va, vb);
    }
    // result (cnt == 1) lives in buffer va: copy into nxt
    std::vector<i64> ident(Nout);
    for (i64 o = 0; o < Nout; ++o) ident[o] = o;
    const int64_t* did = upload(ident.data(), ident.size());
    Act vres = act_of(va), y = act_of(nxt);
    add_op(lname + ".out", [vres, Nout, y, did, crt, B](hipStream_t st) {
        launch_copy_gather(vres, Nout, y, Nout, did, crt, B, st);
    });
    set_out(w, g, Nout, nxt);
}

// gadgets.h ArgMaxPlan. The (K, P) input is level 0's candidate buffer as it stands; later levels ping-pong between
// bufs 2 / 3 (values / index labels) and the ArgMax scratch; the root writes its index labels into the layer's
// output buffer.
void HipEvaluator::plan_argmax(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    DASH_CHECK(hard_, "the ArgMax layer exists in the hardened encoding only");
    const i64 K = g.param("K"), P = g.param("P");
    DASH_CHECK(K >= 2 && K * P == w.N, "argmax input size mismatch");
    const ArgMaxPlan ap(crt_, K);
    if (!amb_[0].p[0]) {
        for (auto& ab : amb_)
            for (int j = 0; j < k_; ++j) {
                const size_t count = static_cast<size_t>(B_) * w.caps.widest[j] * w.caps.maxArgSlots + 64;
                ab.p[j] = dalloc<act_t>(count);
                HIPCHECK(hipMemset(ab.p[j], 0, count * sizeof(act_t)));
            }
        am_hi_ = dalloc<u128>(static_cast<size_t>(B_) * k_ * w.caps.maxSignN);
        am_coli_ = dalloc<uint16_t>(static_cast<size_t>(B_) * k_ * w.caps.maxSignN);
    }
    ensure_ks(w, 1);
    ensure_mrs_ps(w);
    const CrtInfo crt = w.crt;
    const Env e = w.env;
    const int B = B_;
    Act V = act_of(w.cur), I = act_of(3);
    const Act D = amb_[2], E = amb_[3];
    for (int lv = 0; lv < ap.levels(); ++lv) {
        const bool root = ap.root(lv), l0 = lv == 0;
        const int ops = ap.ops[lv], cnt = ap.cnt[lv];
        const i64 Nops = P * ops;
        const std::string pre = arr_name("lv", lv, ".");
        const std::string op = lname + ".lv" + std::to_string(lv);
        // outputs: values into buf 2 / scratch 0, index labels into buf 3 / scratch 1, alternating
        const Act NV = (lv % 2 == 0) ? act_of(2) : amb_[0];
        const Act NI = root ? act_of(w.nxt()) : ((lv % 2 == 0) ? act_of(3) : amb_[1]);
        ArgMaxArgs a{};
        a.crt = crt;
        a.P = P;
        a.ops = ops;
        a.cnt = cnt;
        a.cnt1 = ap.cnt[lv + 1];
        a.pubq = ap.pub[lv][cnt - 1] >= 0 && cnt % 2 == 0 ? ops - 1 : -1;
        a.carry_idx = cnt % 2 == 1 && ap.pub[lv][cnt - 1] < 0;
        a.ks = ks_[0];
        a.hx = hx_;
        a.colx = colx_;
        a.hi = am_hi_;
        a.coli = am_coli_;
        a.vgate0 = gate_base(li + 1, 21 + 3 * lv);
        a.igate0 = gate_base(li + 1, 22 + 3 * lv);
        if (!root) {
            a.gtab = upload_tables(li, pre + "mm.g");
            a.etab = upload_tables(li, pre + "mm.e");
        }
        if (l0) {
            a.itab = upload_tables(li, pre + "idx");
        } else {
            a.igtab = upload_tables(li, pre + "im.g");
            a.ietab = upload_tables(li, pre + "im.e");
        }
        // the sign of the value difference (ArgMaxPlan::sign is the SignMrsPlan of the CRT base), label kept in ks;
        // no y-row pads: the multiply derives the pads of both gate sets from the label
        const MrsArgs s = mrs_sign_args(w, li, pre + "mrs", Nops, gate_base(li + 1, 20 + 3 * lv), a.vgate0, 0, ks_[0]);
        add_op(op + ".diff", [V, D, P, ops, cnt, crt, B](hipStream_t st) {
            launch_argmax_diff(V, D, P, ops, cnt, -1, crt, B, st);
        });
        if (!l0) {
            const int pubq = a.pubq;
            add_op(op + ".idiff", [I, E, P, ops, cnt, pubq, crt, B](hipStream_t st) {
                launch_argmax_diff(I, E, P, ops, cnt, pubq, crt, B, st);
            });
        }
        if (!root) {
            u128* hx = hx_;
            uint16_t* colx = colx_;
            const uint64_t vg = a.vgate0;
            add_op(op + ".H", [D, crt, Nops, hx, colx, vg, e](hipStream_t st) {
                launch_argmax_hash(D, crt, Nops, hx, colx, vg, e.B, e.mc, e.ag, st);
            });
        }
        if (!l0) {
            u128* hi = am_hi_;
            uint16_t* coli = am_coli_;
            const uint64_t ig = a.igate0;
            add_op(op + ".iH", [E, crt, Nops, hi, coli, ig, e](hipStream_t st) {
                launch_argmax_hash(E, crt, Nops, hi, coli, ig, e.B, e.mc, e.ag, st);
            });
        }
        add_op(op + ".mrs", [s, D, e](hipStream_t st) { launch_clip_sign_mrs(s, D, e.B, e.mc, e.ag, st); });
        add_op(op + ".C", [a, root, l0, V, D, I, E, NV, NI, e](hipStream_t st) {
            launch_argmax_mult(a, !root, l0, V, D, I, E, NV, NI, e.B, e.mc, st);
        });
        V = NV;
        I = NI;
    }
    set_out(w, g, P, w.nxt());
}

void HipEvaluator::plan_sumpool(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    PoolGeom G(g.p);
    const CrtInfo crt = w.crt;
    const int B = B_;
    Act x = act_of(w.cur), y = act_of(w.nxt());
    if (G.padded()) {
        // ragged windows: the geometry-direct kernel skips the taps outside the image
        const PoolArgs pa{static_cast<int>(G.C),  static_cast<int>(G.H),  static_cast<int>(G.W),
                          static_cast<int>(G.kh), static_cast<int>(G.kw), static_cast<int>(G.sh),
                          static_cast<int>(G.sw), static_cast<int>(G.ph), static_cast<int>(G.pw),
                          static_cast<int>(G.OH), static_cast<int>(G.OW)};
        DASH_CHECK(G.C * G.H * G.W == w.N, "sumpool input size mismatch");
        add_op(lname + ".geom", [x, y, pa, crt, B](hipStream_t st) { launch_pool_sum(x, y, pa, crt, B, st); });
    } else {
        std::vector<i64> idx, win;
        for (i64 o = 0; o < G.out_size(); ++o) {
            G.window(o, win);
            idx.insert(idx.end(), win.begin(), win.end());
        }
        const int64_t* didx = upload(idx.data(), idx.size());
        const i64 NN = w.N, No = G.out_size();
        const int K = static_cast<int>(G.kh * G.kw);
        add_op(lname, [x, NN, y, No, didx, K, crt, B](hipStream_t st) { launch_window_sum(x, NN, y, No, didx, K, crt, B, st); });
    }
    set_out(w, g, G.out_size(), w.nxt());
}

void HipEvaluator::plan_add(Walk& w, size_t, const GLayer& g, const std::string& lname) {
    const i64 src = g.param("src");
    const auto& s = saved_[src + 1];
    DASH_CHECK(!s.empty(), "residual source not saved");
    Act x = act_of(w.cur), y{};
    for (int j = 0; j < k_; ++j) y.p[j] = s[j];
    const i64 NN = w.N;
    const CrtInfo crt = w.crt;
    const int B = B_;
    add_op(lname, [x, y, NN, crt, B](hipStream_t st) { launch_add(x, y, NN, crt, B, st); });
    set_out(w, g, w.N, w.cur);
}

// operands are saved copies (also the previous layer's output); each goes to its element offset
void HipEvaluator::plan_concat(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const auto& srcs = g.vec("srcs");
    DASH_CHECK(!srcs.empty(), "concat: no operands");
    i64 Ntot = 0;
    for (i64 s : srcs) {
        DASH_CHECK(s >= -1 && s < static_cast<i64>(li) && !saved_[s + 1].empty(), "concat source not saved");
        DASH_CHECK(w.saved_mods[s + 1] == w.saved_mods[srcs[0] + 1], "concat: operands on different moduli");
        Ntot += w.saved_n[s + 1];
    }
    w.mods = w.saved_mods[srcs[0] + 1];
    const CrtInfo ci = crt_info(w.mods);
    Act y = act_of(w.nxt());
    const int B = B_;
    i64 off = 0;
    for (i64 s : srcs) {
        Act x{};
        for (int j = 0; j < k_; ++j) x.p[j] = saved_[s + 1][j];
        const i64 Ns = w.saved_n[s + 1], o = off;
        add_op(lname, [x, Ns, y, Ntot, o, ci, B](hipStream_t st) {
            launch_concat_copy(x, Ns, y, Ntot, o, ci, B, st);
        });
        off += Ns;
    }
    set_out(w, g, Ntot, w.nxt());
}

void HipEvaluator::plan_proj(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    const auto& inm = g.vec("in_mod");
    const auto& outm = g.vec("out_mod");
    ProjArgs a{};
    a.k = k_;
    a.N = w.N;
    a.hard = hard_ ? 1 : 0;
    a.gate0 = gate_base(li + 1, 1);
    for (int j = 0; j < k_; ++j) {
        a.pin[j] = static_cast<int>(inm[j]);
        a.pout[j] = static_cast<int>(outm[j]);
        a.tab[j] = upload_tables(li, arr_name("t.", j, ""));
        w.mods[j] = a.pout[j];
    }
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const Env e = w.env;
    add_op(lname, [a, x, y, e](hipStream_t st) { launch_proj(a, x, y, e.B, e.mc, e.ag, st); });
    set_out(w, g, w.N, w.nxt());
}

void HipEvaluator::plan_mult(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    MultArgs a{};
    a.crt = w.crt;
    a.No = w.N / 2;
    a.hard = hard_ ? 1 : 0;
    a.gate0 = gate_base(li + 1, 1);
    a.q = g.kind == K_MMULT ? static_cast<int>(g.param("q")) : 0;
    if (a.q) a.t = upload_tables(li, "t");
    a.g = upload_tables(li, "g");
    a.e = upload_tables(li, "e");
    Act x = act_of(w.cur), y = act_of(w.nxt());
    const Env e = w.env;
    add_op(lname, [a, x, y, e](hipStream_t st) { launch_mult(a, x, y, e.B, e.mc, e.ag, st); });
    set_out(w, g, a.No, w.nxt());
}

// gadgets.h MulPlan: x = the current activation, y = the saved copy of layer src's output (save_if_needed's own
// buffer, written by its "save" op every run, eagerly and in a replayed graph alike), read in place
void HipEvaluator::plan_mul(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    DASH_CHECK(hard_, "the Mul layer exists in the hardened encoding only");
    DASH_CHECK(w.mods == crt_, "mul: the input is not on the CRT base");
    const bool sq = g.param("sq", 0) != 0;
    MulArgs a{};
    a.crt = w.crt;
    a.N = w.N;
    a.gate0 = gate_base(li + 1, 1);
    Act x = act_of(w.cur), y = act_of(w.nxt()), ys{};
    if (sq) {
        a.Ny = w.N;
        a.g = upload_tables(li, "t");
    } else {
        const i64 src = g.param("src");
        DASH_CHECK(src >= -1 && src < static_cast<i64>(li) && !saved_[src + 1].empty(), "mul: operand not saved");
        DASH_CHECK(w.saved_mods[src + 1] == crt_, "mul: the operand is not on the CRT base");
        a.bc = g.param("bc", 0);
        a.Ny = w.saved_n[src + 1];
        DASH_CHECK(a.bc >= 0 && (a.bc ? (w.N % a.bc == 0 && a.Ny == w.N / a.bc) : a.Ny == w.N),
                   "mul: operand size mismatch");
        for (int j = 0; j < k_; ++j) ys.p[j] = saved_[src + 1][j];
        ys.N = a.Ny;
        a.g = upload_tables(li, "g");
        a.e = upload_tables(li, "e");
    }
    const Env e = w.env;
    add_op(lname, [a, sq, x, ys, y, e](hipStream_t st) { launch_mul(a, sq, x, ys, y, e.B, e.mc, st); });
    set_out(w, g, w.N, w.nxt());
}

// gadgets.h MatMulPlan: x = the current activation (M x T), y = the saved copy of layer src's output (T x N), each G
// head slabs of that shape, read in place as plan_mul reads it; a src that is the layer's own input reads the current
// activation. The key pre-pass compresses every element of both operands once; the contraction reads only the keys
// and colours.
void HipEvaluator::plan_matmul(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    DASH_CHECK(hard_, "the MatMul layer exists in the hardened encoding only");
    DASH_CHECK(w.mods == crt_, "matmul: the input is not on the CRT base");
    const MatMulPlan mp(crt_, g.param("M"), g.param("T"), g.param("N"), g.param("ta", 0) != 0, g.param("tb", 0) != 0,
                        g.param("G", 1));
    const i64 src = g.param("src");
    DASH_CHECK(src >= -1 && src < static_cast<i64>(li) && !saved_[src + 1].empty(), "matmul: operand not saved");
    DASH_CHECK(w.saved_mods[src + 1] == crt_, "matmul: the operand is not on the CRT base");
    DASH_CHECK(w.N == mp.nx() && w.saved_n[src + 1] == mp.ny(), "matmul: operand size mismatch");
    const Array& ga = g.arr("g");
    const Array& ea = g.arr("e");
    DASH_CHECK(ga.shape.size() == 2 && ga.shape[0] == mp.nout() * mp.T && ga.shape[1] == w.crt.sum &&
                   ea.shape == ga.shape, "matmul: table shape");
    ensure_matmul();
    MatMulArgs a{};
    a.crt = w.crt;
    a.M = mp.M;
    a.T = mp.T;
    a.N = mp.N;
    a.G = mp.G;
    a.xsi = mp.xsi;
    a.xst = mp.xst;
    a.yst = mp.yst;
    a.ysl = mp.ysl;
    a.kx = mm_kx_;
    a.ky = mm_ky_;
    a.cx = mm_cx_;
    a.cy = mm_cy_;
    a.gate0 = gate_base(li + 1, 1);
    for (int j = 0; j < k_; ++j)
        if (crt_[j] != 2) a.lds_n = std::max(a.lds_n, nr_comps(crt_[j]));
    a.g = upload_tables(li, "g");
    a.e = upload_tables(li, "e");
    Act x = act_of(w.cur), y = act_of(w.nxt()), ys{};
    const i64 x_src = g.p.count("in_src") ? g.param("in_src") : static_cast<i64>(li) - 1;
    if (src == x_src) {
        ys = x;
    } else {
        for (int j = 0; j < k_; ++j) ys.p[j] = saved_[src + 1][j];
    }
    ys.N = mp.ny();
    // The grid rule: the blocked form where at least one kMmI x kMmL tile is full, else the lane form (a tile of a
    // thinner product would be mostly idle lanes). It is taken per head: a tile never spans heads, so M and N here
    // are a head's. DASH_MATMUL_FORM=lane|blocked overrides it (A/B runs).
    a.blocked = mp.M >= kMmI && mp.N >= kMmL;
    // Heads whose tiles are half full in M (kMmI / 2 <= M < kMmI, N >= kMmL) also take the blocked form while the
    // lane form's grid would leave the device partly filled: at least one block per CU, fewer than the 5 a CU holds
    // (5 waves per SIMD, 4 SIMDs, 4 waves per block). There the idle half of a tile costs nothing and a lane's shared
    // x digits win (docs/MATMUL.md, Heads: (4, 8, 16, 16) against (4, 8, 64, 64)); with fewer blocks than CUs
    // nothing was measured and the per-head rule stands.
    if (mp.G > 1 && !a.blocked && 2 * mp.M >= kMmI && mp.N >= kMmL) {
        const i64 lane_blocks = (mp.nout() + 255) / 256 * k_ * B_;
        a.blocked = lane_blocks >= num_cus() && lane_blocks < 5 * static_cast<i64>(num_cus());
    }
    if (const char* f = std::getenv("DASH_MATMUL_FORM")) {
        if (std::string(f) == "lane") a.blocked = 0;
        if (std::string(f) == "blocked") a.blocked = 1;
    }
    const Env e = w.env;
    const i64 nx = mp.nx(), ny = mp.ny();
    // All MatMul layers share the key buffers: the ops of one evaluator run in order on one stream (or as one chain
    // of a captured graph), so a layer's contraction has read them before the next layer's pre-pass writes them.
    u128 *kxw = mm_kx_, *kyw = mm_ky_;
    uint16_t *cxw = mm_cx_, *cyw = mm_cy_;
    const bool same = src == x_src;  // x x^T: one tensor, keyed once
    if (same) {
        a.ky = a.kx;
        a.cy = a.cx;
    }
    add_op(lname + ".K", [a, x, ys, nx, ny, e, kxw, kyw, cxw, cyw, same](hipStream_t st) {
        launch_label_key(a.crt, nx, kxw, cxw, x, e.B, e.mc, st);
        if (!same) launch_label_key(a.crt, ny, kyw, cyw, ys, e.B, e.mc, st);
    });
    add_op(lname, [a, y, e](hipStream_t st) { launch_matmul(a, y, e.B, e.mc, st); });
    set_out(w, g, mp.nout(), w.nxt());
}

void HipEvaluator::plan_base_ext(Walk& w, size_t li, const GLayer& g, const std::string& lname) {
    std::vector<int> ext;
    for (auto v : g.vec("extra")) ext.push_back(static_cast<int>(v));
    BEPlan be(crt_, ext);
    Act x = act_of(w.cur);
    const Env e = w.env;
    for (int xi : be.extra_idx) {  // the extension's target residues start from the zero label
        RescaleArgs ra{};
        ra.crt = w.crt;
        ra.N = w.N;
        ra.fi = xi;
        ra.up = zero_rows_;
        set_label_rows(ra);
        add_op(lname + ".zero", [ra, x, e](hipStream_t st) { launch_rescale_update(ra, x, e.B, e.mc, st); });
    }
    const BEArgs ba = be_args(w, be, li, "be", w.N, gate_base(li + 1, 1));
    add_op(lname, [ba, x, e](hipStream_t st) { launch_base_ext(ba, x, e.B, e.mc, e.ag, st); });
    set_out(w, g, w.N, w.cur);
}

// ---------------------------------------------------------------------------
// Garbler side of online message #1 on the device. The garbler's secrets for a GC's inputs (the base labels W0
// and the offsets R_p) are placed on the evaluator's GPU once, offline; encode then writes the encoded input
// W0 + x R straight into an evaluator slot's input activations (k_encode_in): only the plaintext input (8 B per
// element) crosses PCIe, and neither side compresses, stages or decompresses a label. This is the in-process form
// of the same-node device transport (IpcTables): the write target is the evaluator's, the labels are the
// garbler's, and the evaluator never reads W0 or R. An encoder holds `slots` GCs (one per evaluator slot of a
// group): encode_all writes all of them with one H2D and one launch.
class DeviceInputEncoder {
   public:
    // g arms encoder slot `slot` (the evaluator slot its tables went to); every other slot stays empty until
    // load() arms it with its own GC (encode refuses empty slots)
    DeviceInputEncoder(const Garbler& g, int device, int slots, int slot = 0)
        : dev_(device), S_(slots), crt_(g.crt()) {
        const CrtLabels& W0 = g.input_base();
        DASH_CHECK(S_ >= 1, "DeviceInputEncoder: slots must be >= 1");
        DASH_CHECK(!W0.empty() && W0.size() == crt_.size(), "DeviceInputEncoder: garble() must run first");
        DASH_CHECK(static_cast<int>(crt_.size()) <= kMaxRes, "DeviceInputEncoder: too many residues");
        bind_device(dev_, nullptr, "DeviceInputEncoder");
        N_ = W0[0].N;
        DASH_CHECK(N_ * 128 < (i64(1) << 31), "DeviceInputEncoder: input too large for the 32-bit lane index");
        a_.k = static_cast<int>(crt_.size());
        size_t off = 0;
        for (size_t j = 0; j < crt_.size(); ++j) {
            const Labels& L = W0[j];
            DASH_CHECK(L.p <= kActMaxModulus, "DeviceInputEncoder: modulus above the byte activations");
            a_.p[j] = L.p;
            a_.n[j] = L.n;
            w_off_.push_back(off);
            off += static_cast<size_t>(L.n) * N_;
            r_off_.push_back(off);
            off += L.n;
        }
        bytes_ = (off + 15) & ~size_t(15);
        a_.wstride = static_cast<int64_t>(bytes_);
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&w_), bytes_ * S_));
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&w_h_), bytes_));
        for (size_t j = 0; j < crt_.size(); ++j) {
            a_.w0[j] = w_ + w_off_[j];
            a_.r[j] = w_ + r_off_[j];
        }
        HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&x_h_), sizeof(int64_t) * N_ * S_));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&x_d_), sizeof(int64_t) * N_ * S_));
        HIPCHECK(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
        HIPCHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
        loaded_.assign(S_, 0);
        load(g, slot);
    }
    ~DeviceInputEncoder() {
        (void)hipSetDevice(dev_);
        if (pending_) (void)hipEventSynchronize(done_);
        (void)hipStreamSynchronize(st_);
        (void)hipStreamDestroy(st_);
        (void)hipEventDestroy(done_);
        (void)hipFree(w_);
        (void)hipFree(x_d_);
        (void)hipHostFree(x_h_);
        (void)hipHostFree(w_h_);
        // teardown errors are ignored (e.g. done_'s last stream capturing in another thread): clear the thread's
        // last error so a later, unrelated HIPCHECK(hipGetLastError()) does not report it
        (void)hipGetLastError();
    }
    DeviceInputEncoder(const DeviceInputEncoder&) = delete;
    DeviceInputEncoder& operator=(const DeviceInputEncoder&) = delete;
    i64 input_size() const { return N_; }
    int slots() const { return S_; }
    // (re-)arm slot s with GC g of the same circuit and base (a serving slot's next GC): its base labels and
    // offsets replace the slot's current ones once the last encode has read them (synchronous, private stream).
    // Concurrent loads of different slots serialize on the shared host staging.
    void load(const Garbler& g, int s) {
        const CrtLabels& W0 = g.input_base();
        DASH_CHECK(s >= 0 && s < S_, "DeviceInputEncoder: slot out of range");
        DASH_CHECK(g.crt() == crt_ && !W0.empty() && W0[0].N == N_, "DeviceInputEncoder: another circuit or base");
        std::lock_guard<std::mutex> lk(load_mu_);
        bind_device(dev_, nullptr, "DeviceInputEncoder.load");
        if (pending_) HIPCHECK(hipEventSynchronize(done_));
        for (size_t j = 0; j < crt_.size(); ++j) {
            const Labels& L = W0[j];
            const comp_t* R = g.offsets().get(L.p);
            act_t* w = w_h_ + w_off_[j];
            for (i64 e = 0; e < N_; ++e)
                for (int c = 0; c < L.n; ++c) w[static_cast<size_t>(c) * N_ + e] = static_cast<act_t>(L.c[e * L.n + c]);
            for (int c = 0; c < L.n; ++c) w_h_[r_off_[j] + c] = static_cast<act_t>(R[c]);
        }
        HIPCHECK(hipMemcpyAsync(w_ + bytes_ * s, w_h_, bytes_, hipMemcpyHostToDevice, st_));
        HIPCHECK(hipStreamSynchronize(st_));
        loaded_[s] = 1;
    }
    // slots [0, n) <- x[n][N] into evaluator slots b0 .. b0 + n - 1, async on st (ordered before h.run on st)
    void encode(HipEvaluator& h, int b0, const i64* x, int n, i64 N, hipStream_t st) {
        DASH_CHECK(N == N_ && h.input_size() == N_, "DeviceInputEncoder: input size mismatch");
        DASH_CHECK(n >= 1 && n <= S_ && b0 >= 0 && b0 + n <= h.batch(), "DeviceInputEncoder: slot range mismatch");
        DASH_CHECK(h.crt() == crt_, "DeviceInputEncoder: the evaluator's CRT base differs from the garbler's");
        DASH_CHECK(h.device() == dev_, "DeviceInputEncoder: the evaluator lives on another device");
        for (int s = 0; s < n; ++s) DASH_CHECK(loaded_[s], "DeviceInputEncoder: slot " + std::to_string(s) + " has no GC");
        bind_device(dev_, st, "DeviceInputEncoder.encode");
        if (pending_) HIPCHECK(hipEventSynchronize(done_));  // the previous H2D has read the pinned staging
        std::memcpy(x_h_, x, sizeof(int64_t) * N_ * n);
        HIPCHECK(hipMemcpyAsync(x_d_, x_h_, sizeof(int64_t) * N_ * n, hipMemcpyHostToDevice, st));
        EncIn a = a_;
        for (int j = 0; j < a.k; ++j) a.out[j] = h.input_act(b0, j);
        launch_encode_in(a, x_d_, N_, n, st);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(done_, st));
        pending_ = true;
    }

   private:
    int dev_, S_;
    std::vector<int> crt_;
    i64 N_ = 0;
    EncIn a_{};
    std::vector<size_t> w_off_, r_off_;
    std::vector<int> loaded_;
    size_t bytes_ = 0;
    act_t* w_ = nullptr;
    act_t* w_h_ = nullptr;
    hipStream_t st_ = nullptr;
    std::mutex load_mu_;
    int64_t* x_h_ = nullptr;
    int64_t* x_d_ = nullptr;
    hipEvent_t done_ = nullptr;
    bool pending_ = false;
};

// ---------------------------------------------------------------------------
namespace {
py::list labels_to_py2(const CrtLabels& L) {
    py::list out;
    for (const auto& x : L) {
        py::array_t<int16_t> arr({static_cast<py::ssize_t>(x.N), static_cast<py::ssize_t>(x.n)});
        std::memcpy(arr.mutable_data(), x.c.data(), x.c.size() * sizeof(comp_t));
        out.append(py::make_tuple(x.p, arr));
    }
    return out;
}
CrtLabels labels_from_py2(const py::list& l) {
    CrtLabels out;
    for (auto item : l) {
        py::tuple t = item.cast<py::tuple>();
        int p = t[0].cast<int>();
        auto arr = py::array_t<int16_t, py::array::c_style | py::array::forcecast>::ensure(t[1]);
        DASH_CHECK(arr && arr.ndim() == 2, "labels must be (N, n) int16 arrays");
        Labels L(p, arr.shape(0));
        DASH_CHECK(arr.shape(1) == L.n, "label width does not match modulus");
        std::memcpy(L.c.data(), arr.data(), L.c.size() * sizeof(comp_t));
        out.push_back(std::move(L));
    }
    return out;
}
hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace

void register_guard_bindings(py::module_& m);  // guard.hip

void register_hip_bindings(py::module_& m) {
    register_guard_bindings(m);
    m.def("encode_compressed_into", [](const Garbler& g, py::array_t<i64, py::array::c_style | py::array::forcecast> x,
                                       HipEvaluator& h, int b) {
        DASH_CHECK(x.size() == h.input_size(), "input size mismatch");
        u128* dst = h.input_slot_compressed(b);
        const i64* xp = x.data();
        const i64 N = x.size();
        py::gil_scoped_release rel;
        g.encode_compressed(xp, N, dst);
    });
    py::class_<DeviceInputEncoder>(m, "DeviceInputEncoder")
        .def(py::init<const Garbler&, int, int, int>(), py::arg("garbler"), py::arg("device"), py::arg("slots") = 1,
             py::arg("slot") = 0)
        .def("input_size", &DeviceInputEncoder::input_size)
        .def("slots", &DeviceInputEncoder::slots)
        .def("load", &DeviceInputEncoder::load, py::arg("garbler"), py::arg("slot") = 0,
             py::call_guard<py::gil_scoped_release>())
        // x: (N,) for one slot or (n, N) for slots 0 .. n - 1 -> evaluator slots b0 ..
        .def("encode_into", [](DeviceInputEncoder& enc, HipEvaluator& h, int b0,
                               py::array_t<i64, py::array::c_style | py::array::forcecast> x, uintptr_t stream) {
            const int n = x.ndim() == 2 ? static_cast<int>(x.shape(0)) : 1;
            const i64 N = x.ndim() == 2 ? static_cast<i64>(x.shape(1)) : static_cast<i64>(x.size());
            DASH_CHECK(x.ndim() == 1 || x.ndim() == 2, "DeviceInputEncoder: x must be (N,) or (slots, N)");
            enc.encode(h, b0, x.data(), n, N, as_stream(stream));
        }, py::arg("evaluator"), py::arg("slot"), py::arg("x"), py::arg("stream") = 0);
    // in-process two-party fast path: the garbler encodes straight into the
    // evaluator's pinned staging slot (the bytes are exactly online message #1)
    m.def("encode_into", [](const Garbler& g, py::array_t<i64, py::array::c_style | py::array::forcecast> x,
                            HipEvaluator& h, int b) {
        auto slot = h.input_slot(b);
        DASH_CHECK(x.size() == h.input_size(), "input size mismatch");
        const i64* xp = x.data();
        const i64 N = x.size();
        py::gil_scoped_release rel;
        g.encode_cm(xp, N, slot);
    });
    // Dedicated non-blocking HIP streams (each new stream is mapped to the next
    // hardware queue), for running independent GC groups concurrently.
    m.def("hip_stream_create", [](int priority) {
        hipStream_t st = nullptr;
        HIPCHECK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority));
        return reinterpret_cast<uintptr_t>(st);
    }, py::arg("priority") = 0);
    m.def("hip_stream_destroy", [](uintptr_t st) { HIPCHECK(hipStreamDestroy(reinterpret_cast<hipStream_t>(st))); });
    m.def("hip_stream_sync", [](uintptr_t st) { HIPCHECK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(st))); });
    // Watchdog primitive: wait for a stream with a deadline instead of an
    // unbounded hipStreamSynchronize (which a hung kernel never returns from).
    // Polls hipStreamQuery with the GIL released; true = drained, false = the
    // deadline passed with work still queued. Errors raised by the stream throw.
    m.def("hip_stream_wait", [](uintptr_t st, double timeout_s) {
        py::gil_scoped_release rel;
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0;; ++spin) {
            const hipError_t e = hipStreamQuery(reinterpret_cast<hipStream_t>(st));
            if (e == hipSuccess) return true;
            if (e != hipErrorNotReady) HIPCHECK(e);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (timeout_s >= 0 && dt > timeout_s) return false;
            if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(spin > 4096 ? 1000 : 50));
        }
    }, py::arg("stream"), py::arg("timeout_s"));
    // Reset the thread's sticky last-error (e.g. after a handled out-of-memory), so a later
    // hipGetLastError() launch check does not report it again. Returns the cleared code.
    m.def("hip_clear_last_error", []() { return static_cast<int>(hipGetLastError()); });
    // Launch planning for tests (launch.h): the CU count the gadget launch pickers plan with (0 restores the
    // device's count; it picks kernel forms, block sizes and grids, never where work runs), and the launch log.
    // An evaluator's picks freeze when its graph is captured: set the count before building the evaluator.
    m.def("hip_set_planning_cus", [](int n) {
        DASH_CHECK(n >= 0, "hip_set_planning_cus: n must be >= 0 (0 restores the device's count)");
        dev::set_planning_cus(n);
    }, py::arg("n"));
    m.def("hip_planning_cus", []() { return dev::num_cus(); });
    m.def("hip_planning_override", []() { return dev::planning_cus_override(); });
    // Joint rescale + ReLU fusion (launch.h joint_fuse): -1 auto (hip_joint_fuse_pick), 0 off, 1 on. Read when an
    // evaluator plans, like the planning count. hip_joint_fuse_pick is the auto rule itself (host arithmetic only)
    // and hip_joint_fuse_min_elems its threshold on batch * N for batches above 2 (INT64_MAX: none takes it).
    m.def("hip_set_joint_fuse", [](int mode) {
        DASH_CHECK(mode >= -1 && mode <= 1, "hip_set_joint_fuse: mode must be -1 (auto), 0 (off) or 1 (on)");
        dev::set_joint_fuse(mode);
    }, py::arg("mode"));
    m.def("hip_joint_fuse", []() { return dev::joint_fuse_mode(); });
    m.def("hip_joint_fuse_pick", [](int64_t N, int B) {
        DASH_CHECK(N >= 1 && B >= 1, "hip_joint_fuse_pick: N and B must be positive");
        return dev::joint_fuse_pick(N, B);
    }, py::arg("N"), py::arg("B"));
    m.def("hip_joint_fuse_min_elems", []() { return dev::joint_fuse_min_elems(); });
    m.def("hip_clip_fuse_pick", [](int64_t N, int B) {
        DASH_CHECK(N >= 1 && B >= 1, "hip_clip_fuse_pick: N and B must be positive");
        return dev::clip_fuse_pick(N, B);
    });
    m.def("hip_launch_log", [](bool on) { dev::launch_log_enable(on); }, py::arg("on"));
    m.def("hip_launch_log_take", []() { return dev::launch_log_take(); });
    // The GPU garbler's own launch record (gpu_garbler.h): a separate list, so the evaluator's log above keeps
    // its contents. hip_garbler_compress_class is host arithmetic only.
    m.def("hip_garbler_log", [](bool on) { gpu_garbler_log_enable(on); }, py::arg("on"));
    m.def("hip_garbler_log_take", []() { return gpu_garbler_log_take(); });
    m.def("hip_garbler_compress_class", [](int q) { return gpu_garbler_compress_class(q); }, py::arg("q"));
    // The conv kernel plan of a dense-conv layer, exactly as the evaluator (mfma: its switch) and the GPU garbler
    // plan it (launch.h conv_layer_plan). Host arithmetic only: works without a device.
    // dh, dw: dilation (a kernel axis of size 1 normalises its dilation to 1, as ConvGeom does). The result also
    // names the dilation the kernel form is picked by (dil), the input rows of a full band (band_input_rows, the
    // launch's dynamic LDS is that times ldsR) and the LDS bytes staged per image over all bands (staged_bytes).
    m.def("hip_conv_plan", [](int C, int H, int W, int F, int kh, int kw, int sh, int sw, int ph, int pw,
                              const std::vector<int>& crt_moduli, bool mfma, int dh, int dw) {
        DASH_CHECK(C > 0 && H > 0 && W > 0 && F > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0,
                   "hip_conv_plan: bad conv geometry");
        DASH_CHECK(dh >= 1 && dw >= 1, "hip_conv_plan: dilation must be at least 1");
        if (kh == 1) dh = 1;
        if (kw == 1) dw = 1;
        DASH_CHECK(!crt_moduli.empty() && static_cast<int>(crt_moduli.size()) <= dev::kMaxRes,
                   "hip_conv_plan: 1 .. 16 CRT moduli");
        dev::ConvArgs a{};
        a.crt.k = static_cast<int>(crt_moduli.size());
        for (int j = 0; j < a.crt.k; ++j) {
            DASH_CHECK(crt_moduli[j] >= 2, "hip_conv_plan: modulus below 2");
            a.crt.p[j] = crt_moduli[j];
            a.crt.n[j] = nr_comps(crt_moduli[j]);
        }
        a.C = C; a.H = H; a.W = W; a.F = F; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
        a.dh = dh; a.dw = dw;
        DASH_CHECK(H + 2 * ph >= (kh - 1) * dh + 1 && W + 2 * pw >= (kw - 1) * dw + 1, "hip_conv_plan: empty output");
        a.OH = (H + 2 * ph - (kh - 1) * dh - 1) / sh + 1;
        a.OW = (W + 2 * pw - (kw - 1) * dw - 1) / sw + 1;
        DASH_CHECK(a.OH > 0 && a.OW > 0, "hip_conv_plan: empty output");
        dev::conv_layer_plan(a, mfma && dev::conv_img_enabled());
        py::dict d;
        d["ur"] = a.ur;
        d["KS"] = a.kh * a.kw * (a.Cpad / 64);
        d["Cpad"] = a.Cpad;
        d["Kpad"] = a.Kpad;
        d["ldsS"] = a.ldsS;
        d["ldsR"] = a.ldsR;
        d["band"] = a.band;
        d["nbands"] = a.nbands;
        d["OH"] = a.OH;
        d["OW"] = a.OW;
        d["sh24"] = std::vector<int>(a.sh24, a.sh24 + a.crt.k);
        d["dil"] = dev::conv_dilated(a) ? 1 : 0;
        d["band_input_rows"] = a.nbands > 0 ? dev::conv_band_in_rows(std::min(a.band, a.OH), a.sh, a.kh, a.dh) : 0;
        int64_t staged = 0;
        for (int b = 0; b < a.nbands; ++b)
            staged += static_cast<int64_t>(dev::conv_band_in_rows(std::min(a.band, a.OH - b * a.band), a.sh, a.kh, a.dh)) *
                      a.ldsR;
        d["staged_bytes"] = staged;
        return d;
    }, py::arg("C"), py::arg("H"), py::arg("W"), py::arg("F"), py::arg("kh"), py::arg("kw"), py::arg("sh"),
       py::arg("sw"), py::arg("ph"), py::arg("pw"), py::arg("crt_moduli"), py::arg("mfma") = true, py::arg("dh") = 1,
       py::arg("dw") = 1);
    // The grouped conv's block geometry (launch.h conv_grp_geometry), as plan_conv and the GPU garbler plan it
    m.def("hip_conv_grp_plan", [](int C, int H, int W, int F, int kh, int kw, int sh, int sw, int ph, int pw,
                                  int groups, const std::vector<int>& crt_moduli, int dh, int dw) {
        DASH_CHECK(C > 0 && H > 0 && W > 0 && F > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0,
                   "hip_conv_grp_plan: bad conv geometry");
        DASH_CHECK(groups > 1 && C % groups == 0 && F % groups == 0, "hip_conv_grp_plan: groups > 1 dividing C and F");
        DASH_CHECK(dh >= 1 && dw >= 1, "hip_conv_grp_plan: dilation must be at least 1");
        DASH_CHECK(!crt_moduli.empty() && static_cast<int>(crt_moduli.size()) <= dev::kMaxRes,
                   "hip_conv_grp_plan: 1 .. 16 CRT moduli");
        if (kh == 1) dh = 1;
        if (kw == 1) dw = 1;
        dev::ConvArgs a{};
        a.crt.k = static_cast<int>(crt_moduli.size());
        for (int j = 0; j < a.crt.k; ++j) {
            DASH_CHECK(crt_moduli[j] >= 2, "hip_conv_grp_plan: modulus below 2");
            a.crt.p[j] = crt_moduli[j];
            a.crt.n[j] = nr_comps(crt_moduli[j]);
        }
        a.C = C; a.H = H; a.W = W; a.F = F; a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
        a.dh = dh; a.dw = dw;
        a.groups = groups;
        DASH_CHECK(H + 2 * ph >= (kh - 1) * dh + 1 && W + 2 * pw >= (kw - 1) * dw + 1,
                   "hip_conv_grp_plan: empty output");
        a.OH = (H + 2 * ph - (kh - 1) * dh - 1) / sh + 1;
        a.OW = (W + 2 * pw - (kw - 1) * dw - 1) / sw + 1;
        const size_t lds = dev::conv_grp_geometry(a);
        py::dict d;
        d["dil"] = dev::conv_dilated(a) ? 1 : 0;
        d["gpb"] = a.gpb;
        d["gngb"] = a.gngb;
        d["gband"] = a.gband;
        d["gnbands"] = a.gnbands;
        d["gR"] = a.gR;
        d["gnpp"] = a.gnpp;
        d["kwd"] = dev::conv_grp_kwd(a.kw, dev::conv_dilated(a));
        d["band_input_rows"] = dev::conv_band_in_rows(a.gband, a.sh, a.kh, a.dh);
        d["lds"] = static_cast<int64_t>(lds);
        d["OH"] = a.OH;
        d["OW"] = a.OW;
        return d;
    }, py::arg("C"), py::arg("H"), py::arg("W"), py::arg("F"), py::arg("kh"), py::arg("kw"), py::arg("sh"),
       py::arg("sw"), py::arg("ph"), py::arg("pw"), py::arg("groups"), py::arg("crt_moduli"), py::arg("dh") = 1,
       py::arg("dw") = 1);
    // The same for a transposed conv: the plan of its sub-pixel view (layers.h ConvTGeom, launch.h
    // convt_view_args) and the scatter description, as plan_convt and the GPU garbler build them.
    m.def("hip_convt_plan", [](int C, int H, int W, int F, int kh, int kw, int sh, int sw, int ph, int pw, int oph,
                               int opw, const std::vector<int>& crt_moduli, bool mfma) {
        DASH_CHECK(!crt_moduli.empty() && static_cast<int>(crt_moduli.size()) <= dev::kMaxRes,
                   "hip_convt_plan: 1 .. 16 CRT moduli");
        Params p{{"C", {C}}, {"H", {H}}, {"W", {W}}, {"F", {F}}, {"kh", {kh}}, {"kw", {kw}}, {"sh", {sh}},
                 {"sw", {sw}}, {"ph", {ph}}, {"pw", {pw}}, {"oph", {oph}}, {"opw", {opw}}};
        const ConvTGeom G(p);
        dev::ConvArgs a{};
        a.crt.k = static_cast<int>(crt_moduli.size());
        for (int j = 0; j < a.crt.k; ++j) {
            DASH_CHECK(crt_moduli[j] >= 2, "hip_convt_plan: modulus below 2");
            a.crt.p[j] = crt_moduli[j];
            a.crt.n[j] = nr_comps(crt_moduli[j]);
        }
        dev::convt_view_args(a, C, H, W, F, kh, kw, sh, sw, ph, pw, static_cast<int>(G.OH), static_cast<int>(G.OW));
        dev::conv_layer_plan(a, mfma && dev::conv_img_enabled());
        py::dict d;
        d["ur"] = a.ur;
        d["KS"] = a.kh * a.kw * (a.Cpad / 64);
        d["Cpad"] = a.Cpad;
        d["Kpad"] = a.Kpad;
        d["band"] = a.band;
        d["nbands"] = a.nbands;
        d["VF"] = a.F;
        d["VOH"] = a.OH;
        d["VOW"] = a.OW;
        d["Th"] = static_cast<int>(G.Th);
        d["Tw"] = static_cast<int>(G.Tw);
        d["OH"] = a.tOH;
        d["OW"] = a.tOW;
        d["tsc"] = a.tsc;
        return d;
    }, py::arg("C"), py::arg("H"), py::arg("W"), py::arg("F"), py::arg("kh"), py::arg("kw"), py::arg("sh"),
       py::arg("sw"), py::arg("ph"), py::arg("pw"), py::arg("oph"), py::arg("opw"), py::arg("crt_moduli"),
       py::arg("mfma") = true);
    // the view's weights [F sh sw][C][Th][Tw] from w [C][F][kh][kw] (ConvTGeom::view_weights), flat
    m.def("convt_view_weights", [](const std::vector<i64>& w, int C, int F, int kh, int kw, int sh, int sw) {
        Params p{{"C", {C}}, {"H", {1}}, {"W", {1}}, {"F", {F}}, {"kh", {kh}}, {"kw", {kw}}, {"sh", {sh}},
                 {"sw", {sw}}};
        const ConvTGeom G(p);
        DASH_CHECK(static_cast<i64>(w.size()) == G.F * G.K(), "convt_view_weights: weight shape");
        return G.view_weights(w.data());
    }, py::arg("w"), py::arg("C"), py::arg("F"), py::arg("kh"), py::arg("kw"), py::arg("sh"), py::arg("sw"));
    m.def("hip_device_count", []() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) return 0;
        return n;
    });
    // "dddd:bb:dd.f" of a device (multi-GPU bench evidence: which physical GPU each rank ran on)
    m.def("hip_device_pci_bus_id", [](int device) {
        char buf[64] = {0};
        HIPCHECK(hipDeviceGetPCIBusId(buf, static_cast<int>(sizeof(buf)), device));
        return std::string(buf);
    });
    py::class_<IpcTables, std::shared_ptr<IpcTables>>(m, "IpcTables")
        .def(py::init([](int device, const py::list& handles, int B) {
                 std::vector<std::tuple<size_t, std::string, size_t, std::string>> hs;
                 for (auto item : handles) {
                     auto t = item.cast<py::tuple>();
                     hs.emplace_back(t[0].cast<size_t>(), t[1].cast<std::string>(), t[2].cast<size_t>(),
                                     t[3].cast<std::string>());
                 }
                 return std::make_shared<IpcTables>(device, hs, B);
             }),
             py::arg("device"), py::arg("handles"), py::arg("batch"))
        .def("tables", &IpcTables::tables)
        .def("sink", &IpcTables::sink, "slot b of the evaluator's table arenas as a GPU-garbler destination");
    py::class_<HipEvaluator, std::shared_ptr<HipEvaluator>>(m, "HipEvaluator")
        .def(py::init([](std::shared_ptr<GarbledModel> tmpl, int B, int device, bool mfma, bool stream_tables) {
                 return std::make_shared<HipEvaluator>(std::move(tmpl), B, device, mfma, stream_tables);
             }),
             py::arg("template"), py::arg("batch"), py::arg("device") = 0, py::arg("mfma") = true,
             py::arg("stream_tables") = false)
        .def_property_readonly("streams_tables", &HipEvaluator::streams_tables)
        .def("load", [](HipEvaluator& h, int b, std::shared_ptr<GarbledModel> m) {
            py::gil_scoped_release rel;
            h.load(b, *m);
        })
        .def("sink", &HipEvaluator::sink, "slot b's table arenas as a GPU-garbler destination (zero-copy load)")
        .def("ipc_export", [](const HipEvaluator& h) {
            py::list out;
            for (const auto& e : h.ipc_export())
                out.append(py::make_tuple(std::get<0>(e), std::get<1>(e), std::get<2>(e), py::bytes(std::get<3>(e))));
            return out;
        }, "IPC handles of the table arenas: [(layer, table, bytes per slot, handle)] (same-node device transport)")
        .def_property_readonly("batch", &HipEvaluator::batch)
        .def("device_bytes", &HipEvaluator::device_bytes)
        .def("table_bytes", &HipEvaluator::table_bytes)
        .def("set_profile", &HipEvaluator::set_profile)
        .def("op_times", &HipEvaluator::op_times)
        .def("set_inputs", [](HipEvaluator& h, const py::list& inputs, uintptr_t stream) {
            std::vector<CrtLabels> in;
            for (auto it : inputs) in.push_back(labels_from_py2(it.cast<py::list>()));
            h.set_inputs(in, as_stream(stream));
        }, py::arg("inputs"), py::arg("stream") = 0)
        .def("run", [](HipEvaluator& h, uintptr_t stream) { h.run(as_stream(stream)); }, py::arg("stream") = 0)
        .def("set_input_cm", [](HipEvaluator& h, int b, const py::list& arrs) {
            auto slot = h.input_slot(b);
            DASH_CHECK(static_cast<size_t>(py::len(arrs)) == slot.size(), "one array per residue expected");
            for (size_t j = 0; j < slot.size(); ++j) {
                auto a = py::array_t<int16_t, py::array::c_style | py::array::forcecast>::ensure(arrs[j]);
                std::memcpy(slot[j], a.data(), a.size() * sizeof(int16_t));
            }
        })
        .def("upload_inputs", [](HipEvaluator& h, uintptr_t stream) { h.upload_inputs(as_stream(stream)); }, py::arg("stream") = 0)
        .def("set_input_compressed", [](HipEvaluator& h, int b, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> c) {
            DASH_CHECK(c.ndim() == 3 && c.shape(0) == h.crt_size() && c.shape(1) == h.input_size() && c.shape(2) == 2,
                       "compressed inputs must be (k, N, 2) uint64");
            std::memcpy(h.input_slot_compressed(b), c.data(), sizeof(u128) * h.crt_size() * h.input_size());
        })
        .def("upload_inputs_compressed", [](HipEvaluator& h, uintptr_t stream) { h.upload_inputs_compressed(as_stream(stream)); },
             py::arg("stream") = 0)
        .def("fetch_outputs", [](HipEvaluator& h, uintptr_t stream) { h.fetch_outputs(as_stream(stream)); }, py::arg("stream") = 0)
        .def("crt_size", &HipEvaluator::crt_size)
        .def("set_graph", &HipEvaluator::set_graph)
        .def("input_size", &HipEvaluator::input_size)
        .def("output_size", &HipEvaluator::output_size)
        .def("outputs_compressed", [](const HipEvaluator& h, int b) {
            auto r = h.outputs_compressed(b);
            py::array_t<uint64_t> out({static_cast<py::ssize_t>(h.crt_size()), static_cast<py::ssize_t>(h.output_size()),
                                       static_cast<py::ssize_t>(2)});
            std::memcpy(out.mutable_data(), r.data(), r.size() * sizeof(u128));
            return out;
        })
        .def("decode_into", [](const HipEvaluator& h, int b, const Decoder& d) {
            // online message #2 (compressed) decoded by the garbler, no Python round trip
            auto r = h.outputs_compressed(b);
            return d.decode_compressed(r.data());
        })
        .def("get_outputs", [](HipEvaluator& h, uintptr_t stream) {
            auto o = h.get_outputs(as_stream(stream));
            py::list r;
            for (auto& x : o) r.append(labels_to_py2(x));
            return r;
        }, py::arg("stream") = 0)
        .def("evaluate", [](HipEvaluator& h, const py::list& inputs, uintptr_t stream) {
            std::vector<CrtLabels> in;
            for (auto it : inputs) in.push_back(labels_from_py2(it.cast<py::list>()));
            std::vector<CrtLabels> o;
            {
                py::gil_scoped_release rel;
                h.set_inputs(in, as_stream(stream));
                h.run(as_stream(stream));
                o = h.get_outputs(as_stream(stream));
            }
            py::list r;
            for (auto& x : o) r.append(labels_to_py2(x));
            return r;
        }, py::arg("inputs"), py::arg("stream") = 0);

    // parity helpers for tests
    m.def("hip_aes_hash_array", [](py::array_t<uint64_t, py::array::c_style | py::array::forcecast> a) {
        DASH_CHECK(a.ndim() == 2 && a.shape(1) == 2, "expected (n,2) uint64");
        const int64_t n = a.shape(0);
        auto te = make_te0();
        auto rk = fixed_round_key_words();
        uint32_t *dte, *drk;
        u128 *din, *dout;
        HIPCHECK(hipMalloc(&dte, 256 * 4));
        HIPCHECK(hipMalloc(&drk, 44 * 4));
        HIPCHECK(hipMalloc(&din, n * 16 + 16));
        HIPCHECK(hipMalloc(&dout, n * 16 + 16));
        HIPCHECK(hipMemcpy(dte, te.data(), 256 * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(drk, rk.data(), 44 * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(din, a.data(), n * 16, hipMemcpyHostToDevice));
        AesGlobals g{dte, drk};
        launch_aes_test(din, dout, n, g, nullptr);
        py::array_t<uint64_t> out({static_cast<py::ssize_t>(n), static_cast<py::ssize_t>(2)});
        HIPCHECK(hipMemcpy(out.mutable_data(), dout, n * 16, hipMemcpyDeviceToHost));
        (void)hipFree(dte); (void)hipFree(drk); (void)hipFree(din); (void)hipFree(dout);
        return out;
    });
    m.def("hip_hard_pads", [](py::array_t<uint64_t, py::array::c_style | py::array::forcecast> keys,
                              py::array_t<uint64_t, py::array::c_style | py::array::forcecast> gates,
                              py::array_t<uint32_t, py::array::c_style | py::array::forcecast> subs,
                              py::array_t<uint32_t, py::array::c_style | py::array::forcecast> blks) {
        DASH_CHECK(keys.ndim() == 2 && keys.shape(1) == 2, "keys: (n, 2) uint64");
        const int64_t n = keys.shape(0);
        DASH_CHECK(gates.size() == n && subs.size() == n && blks.size() == n, "one gate / sub / block per key");
        u128 *dk, *dout;
        uint64_t* dg;
        uint32_t *ds, *db;
        HIPCHECK(hipMalloc(&dk, n * 16 + 16));
        HIPCHECK(hipMalloc(&dout, n * 64 + 64));
        HIPCHECK(hipMalloc(&dg, n * 8 + 8));
        HIPCHECK(hipMalloc(&ds, n * 4 + 4));
        HIPCHECK(hipMalloc(&db, n * 4 + 4));
        HIPCHECK(hipMemcpy(dk, keys.data(), n * 16, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dg, gates.data(), n * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(ds, subs.data(), n * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(db, blks.data(), n * 4, hipMemcpyHostToDevice));
        launch_hard_test(dk, dg, ds, db, dout, n, nullptr);
        py::array_t<uint64_t> out({static_cast<py::ssize_t>(n), static_cast<py::ssize_t>(4), static_cast<py::ssize_t>(2)});
        HIPCHECK(hipMemcpy(out.mutable_data(), dout, n * 64, hipMemcpyDeviceToHost));
        (void)hipFree(dk); (void)hipFree(dout); (void)hipFree(dg); (void)hipFree(ds); (void)hipFree(db);
        return out;
    }, "hardened-encoding pads computed on the GPU (dev.h hard_block), (n, 4, 2) uint64");
    m.def("hip_aes_bench", [](int blocks, int iters) {
        // returns (ms, AES blocks per second)
        auto te = make_te0();
        uint32_t* dte;
        u128* dout;
        HIPCHECK(hipMalloc(&dte, 256 * 4));
        HIPCHECK(hipMalloc(&dout, static_cast<size_t>(blocks) * 512 * 16));
        HIPCHECK(hipMemcpy(dte, te.data(), 256 * 4, hipMemcpyHostToDevice));
        AesGlobals g{dte, nullptr};
        launch_aes_bench(dout, blocks, 4, g, nullptr);  // warm-up
        hipEvent_t e0, e1;
        HIPCHECK(hipEventCreate(&e0));
        HIPCHECK(hipEventCreate(&e1));
        HIPCHECK(hipEventRecord(e0, nullptr));
        launch_aes_bench(dout, blocks, iters, g, nullptr);
        HIPCHECK(hipEventRecord(e1, nullptr));
        HIPCHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        (void)hipFree(dte); (void)hipFree(dout);
        const double n = 2.0 * iters * blocks * 512.0;
        return py::make_tuple(ms, n / (ms * 1e-3));
    });
    // Constant-modulus kernel forms (launch.h const_mod_mode): 0 none, 1 the joint output kernels, 2 also the staged
    // chain. Read at every host-side launch: set it before an evaluator's first run. hip_chain_const_mod_pick is
    // the staged chain's rule on a base (host arithmetic only); hip_const_mod_launches counts the host-side launches
    // that took a constant form, (staged chain, output kernels).
    m.def("hip_set_const_mod", [](int mode) {
        DASH_CHECK(mode >= 0 && mode <= 2, "hip_set_const_mod: mode must be 0 (off), 1 (output kernels) or 2 (and the chain)");
        dev::set_const_mod(mode);
    });
    m.def("hip_const_mod", []() { return dev::const_mod_mode(); });
    m.def("hip_const_mod_launches", []() {
        return py::make_tuple(dev::const_mod_launches(true), dev::const_mod_launches(false));
    });
    m.def("hip_chain_const_mod_pick", [](const std::vector<int>& primes) {
        return dev::chain_const_mod_pick(primes.data(), static_cast<int>(primes.size()));
    });
    // (q, n, c, D, Dn, v, sh) of dev::ModK<q> (None where q has no constant form) and of the ModC table's entry
    m.def("hip_modk_constants", [](int q) -> py::object {
        ModC k;
        if (!modk_constants(q, k)) return py::none();
        return py::make_tuple(k.q, k.n, k.c, k.D, k.Dn, k.v, k.sh);
    });
    m.def("hip_modc_constants", [](int q) {
        DASH_CHECK(q >= 2 && q < (1 << 16), "hip_modc_constants: modulus out of range");
        const ModC k = make_modc(q);
        return py::make_tuple(k.q, k.n, k.c, k.D, k.Dn, k.v, k.sh);
    });
    m.def("hip_modk_digits", [](int q, py::array_t<uint32_t, py::array::c_style | py::array::forcecast> r) {
        // dev::ModK<q>'s helpers on chunk remainders r < D (k_modk_test): (N, kModkTestRow) uint32 rows
        DASH_CHECK(r.ndim() == 1 && r.shape(0) >= 1, "expected a non-empty 1-d array");
        const int64_t N = r.shape(0);
        const size_t ob = static_cast<size_t>(N) * dev::kModkTestRow * 4;
        struct Bufs {  // freed on every way out
            uint32_t *r = nullptr, *out = nullptr;
            ~Bufs() { (void)hipFree(r); (void)hipFree(out); }
        } d;
        HIPCHECK(hipMalloc(&d.r, N * 4));
        HIPCHECK(hipMalloc(&d.out, ob));
        HIPCHECK(hipMemcpy(d.r, r.data(), N * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d.out, 0, ob));
        launch_modk_test(q, d.r, N, d.out, nullptr);
        py::array_t<uint32_t> out({static_cast<py::ssize_t>(N), static_cast<py::ssize_t>(dev::kModkTestRow)});
        HIPCHECK(hipMemcpy(out.mutable_data(), d.out, ob, hipMemcpyDeviceToHost));
        return out;
    });
    m.def("hip_codec", [](py::array_t<int16_t, py::array::c_style | py::array::forcecast> labels, int q) {
        // labels (N, n) label-major -> (compressed (N,2) u64, decompressed (N, n))
        DASH_CHECK(labels.ndim() == 2, "expected (N, n)");
        const int64_t N = labels.shape(0), n = labels.shape(1);
        DASH_CHECK(n == nr_comps(q), "label width mismatch");
        std::vector<int16_t> cm(N * n);
        for (int64_t e = 0; e < N; ++e)
            for (int64_t c = 0; c < n; ++c) cm[c * N + e] = labels.data()[e * n + c];
        std::vector<ModC> mc(q + 1);
        mc[q] = make_modc(q);
        ModC* dmc;
        int16_t *dl, *dd;
        u128* dc;
        HIPCHECK(hipMalloc(&dmc, sizeof(ModC) * (q + 1)));
        HIPCHECK(hipMalloc(&dl, N * n * 2));
        HIPCHECK(hipMalloc(&dd, N * n * 2));
        HIPCHECK(hipMalloc(&dc, N * 16));
        HIPCHECK(hipMemcpy(dmc, mc.data(), sizeof(ModC) * (q + 1), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dl, cm.data(), N * n * 2, hipMemcpyHostToDevice));
        launch_codec_test(dl, N, q, dmc, dc, dd, nullptr);
        py::array_t<uint64_t> comp({static_cast<py::ssize_t>(N), static_cast<py::ssize_t>(2)});
        HIPCHECK(hipMemcpy(comp.mutable_data(), dc, N * 16, hipMemcpyDeviceToHost));
        std::vector<int16_t> dec(N * n);
        HIPCHECK(hipMemcpy(dec.data(), dd, N * n * 2, hipMemcpyDeviceToHost));
        py::array_t<int16_t> decomp({static_cast<py::ssize_t>(N), static_cast<py::ssize_t>(n)});
        for (int64_t e = 0; e < N; ++e)
            for (int64_t c = 0; c < n; ++c) decomp.mutable_data()[e * n + c] = dec[c * N + e];
        (void)hipFree(dmc); (void)hipFree(dl); (void)hipFree(dd); (void)hipFree(dc);
        return py::make_tuple(comp, decomp);
    });
}

}  // namespace dash
