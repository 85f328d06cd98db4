// host_parity.cc -- replays a scenario file through a MetricSystem (include/loghisto.hpp) and dumps what came out.
// No test logic and no oracle here: tests/test_gpu_host_parity.py writes the scenario, runs this program as a child
// process and compares the dump with the oracle.
//
//   host_parity <scenario file> <dump file>
//
// Exit status: 0 the replay completed (also without a device: Histogram is then a no-op, last_status() says so, counters
// are still replayed); 2 usage or a malformed scenario; 3 the engine could not be created for a reason other than "no
// device" (message on stderr).
//
// Both files are little-endian and packed.  str = u32 length + bytes.
//
// Scenario
//   char[8]  "LHSCN001"
//   u32      max_metrics, num_buffers, num_lanes, stage_samples
//   u64      lane_samples
//   u32      device_counters (0 | 1), max_counters
//   u32      mode: 0 stepped, 1 concurrent
//   u32      wire format (0 none, 1 Graphite, 2 OpenTSDB), histogram_keys_in_map (0 | 1)
//   i32      number of percentiles, -1 = keep the defaults; then per percentile: str label, f64 p
//   u32      number of names; then per name: str
//   u32      T producer threads, S steps (concurrent mode plays step 0 only)
//   u32[S]   per-step flag: 0 do not collect; 1 collect, dump, then release this raw set and every kept one;
//            2 collect, dump and KEEP the raw set unreleased (until a later step with flag 1 has been dumped)
//   then for step 0 .. S-1, for thread 0 .. T-1:
//     u32 n, u8 kind[n] (0 Histogram, 1 Counter), u32 name_index[n], u64 payload[n] (the float64's bits | the amount)
//
//   Stepped: every producer replays its list of step j and arrives at a barrier; the main thread then -- unless the flag
//   is 0 -- calls collectRawMetrics, processMetrics and addAggregates, dumps the interval, releases as the flag says and
//   opens the barrier.  Concurrent: the producers run their lists without barriers while the main thread collects, dumps
//   and releases about every millisecond until all of them have finished; one last collect follows.
//
// Dump
//   char[8]  "LHDMP001"
//   records, each starting with a u32 tag:
//   1 (interval)
//     u32 step (concurrent: a running number), i32 last_status, u64 dropped_intervals, i64 Time in ns since the epoch,
//     u32 has_snapshot
//     u32 n; per name: str name, u32 cells, i16 key[cells], u64 count[cells]          raw->Histograms(), keys ascending
//     u32 n; per entry: str, u64                                                       Rates
//     u32 n; per entry: str, u64                                                       Counters
//     u32 n; per entry: str, u64 float64 bits                                          Gauges
//     u32 n; per entry: str, u64 float64 bits                                          ProcessedMetricSet::Metrics
//     u32 wire_format, str wire
//   2 (end) i32 last_status, u64 dropped_intervals, u32 engine_ready
#include "../../include/loghisto.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>

using namespace loghisto;

namespace {

struct Reader {
    std::vector<uint8_t> b;
    size_t at = 0;
    bool bad = false;
    const uint8_t *take(size_t n)
    {
        if (bad || n > b.size() - at) { bad = true; return nullptr; }
        const uint8_t *p = b.data() + at;
        at += n;
        return p;
    }
    template <class T> T get()
    {
        T v{};
        if (const uint8_t *p = take(sizeof(T))) std::memcpy(&v, p, sizeof(T));
        return v;
    }
    std::string str()
    {
        const uint32_t n = get<uint32_t>();
        const uint8_t *p = take(n);
        return p ? std::string(reinterpret_cast<const char *>(p), n) : std::string();
    }
    template <class T> std::vector<T> array(size_t n)
    {
        std::vector<T> v;
        if (n > (b.size() - at) / sizeof(T)) { bad = true; return v; }
        v.resize(n);
        if (n) std::memcpy(v.data(), take(n * sizeof(T)), n * sizeof(T));
        return v;
    }
};

struct Writer {
    std::FILE *f;
    template <class T> void put(T v) { std::fwrite(&v, sizeof(T), 1, f); }
    void str(const std::string &s)
    {
        put<uint32_t>((uint32_t)s.size());
        std::fwrite(s.data(), 1, s.size(), f);
    }
};

struct Events {
    std::vector<uint8_t> kind;
    std::vector<uint32_t> name;
    std::vector<uint64_t> payload;
};

uint64_t bits_of(double v)
{
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

template <class Map> std::vector<typename Map::const_iterator> sorted(const Map &m)
{
    std::vector<typename Map::const_iterator> it;
    for (auto i = m.begin(); i != m.end(); ++i) it.push_back(i);
    std::sort(it.begin(), it.end(), [](auto a, auto b) { return a->first < b->first; });
    return it;
}

void dump_interval(Writer &w, MetricSystem &ms, uint32_t step, RawMetricSet &raw, const ProcessedMetricSet &pm)
{
    w.put<uint32_t>(1);
    w.put<uint32_t>(step);
    w.put<int32_t>(ms.last_status());
    w.put<uint64_t>(ms.dropped_intervals());
    w.put<int64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(raw.Time.time_since_epoch()).count());
    w.put<uint32_t>(raw.snapshot ? 1u : 0u);
    const auto &h = raw.Histograms();
    w.put<uint32_t>((uint32_t)h.size());
    for (auto it : sorted(h)) {
        w.str(it->first);
        w.put<uint32_t>((uint32_t)it->second.size());
        for (auto &kv : it->second) w.put<int16_t>(kv.first);
        for (auto &kv : it->second) w.put<uint64_t>(kv.second);
    }
    w.put<uint32_t>((uint32_t)raw.Rates.size());
    for (auto it : sorted(raw.Rates)) { w.str(it->first); w.put<uint64_t>(it->second); }
    w.put<uint32_t>((uint32_t)raw.Counters.size());
    for (auto it : sorted(raw.Counters)) { w.str(it->first); w.put<uint64_t>(it->second); }
    w.put<uint32_t>((uint32_t)raw.Gauges.size());
    for (auto it : sorted(raw.Gauges)) { w.str(it->first); w.put<uint64_t>(bits_of(it->second)); }
    w.put<uint32_t>((uint32_t)pm.Metrics.size());
    for (auto it : sorted(pm.Metrics)) { w.str(it->first); w.put<uint64_t>(bits_of(it->second)); }
    w.put<uint32_t>((uint32_t)pm.wire_format);
    w.str(pm.wire);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: host_parity <scenario file> <dump file>\n");
        return 2;
    }
    Reader r;
    {
        std::FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) r.b.insert(r.b.end(), buf, buf + n);
        std::fclose(f);
    }
    const uint8_t *magic = r.take(8);
    if (!magic || std::memcmp(magic, "LHSCN001", 8) != 0) {
        std::fprintf(stderr, "host_parity: %s is not a scenario file\n", argv[1]);
        return 2;
    }
    Options opt;
    opt.max_metrics = r.get<uint32_t>();
    opt.num_buffers = r.get<uint32_t>();
    opt.num_lanes = r.get<uint32_t>();
    opt.stage_samples = r.get<uint32_t>();
    opt.lane_samples = r.get<uint64_t>();
    opt.device_counters = r.get<uint32_t>() != 0;
    opt.max_counters = r.get<uint32_t>();
    const uint32_t mode = r.get<uint32_t>();
    const uint32_t wire = r.get<uint32_t>();
    const bool keys_in_map = r.get<uint32_t>() != 0;
    const int32_t npct = r.get<int32_t>();
    std::map<std::string, double> pct;
    for (int32_t i = 0; i < npct && !r.bad; i++) {
        std::string label = r.str();
        const uint64_t pb = r.get<uint64_t>();
        double p;
        std::memcpy(&p, &pb, 8);
        pct[label] = p;
    }
    const uint32_t nnames = r.get<uint32_t>();
    std::vector<std::string> names;
    for (uint32_t i = 0; i < nnames && !r.bad; i++) names.push_back(r.str());
    const uint32_t T = r.get<uint32_t>(), S = r.get<uint32_t>();
    std::vector<uint32_t> flags = r.array<uint32_t>(S);
    std::vector<std::vector<Events>> script(S); // [step][thread]
    for (uint32_t j = 0; j < S && !r.bad; j++) {
        script[j].resize(T);
        for (uint32_t t = 0; t < T && !r.bad; t++) {
            Events &e = script[j][t];
            const uint32_t n = r.get<uint32_t>();
            e.kind = r.array<uint8_t>(n);
            e.name = r.array<uint32_t>(n);
            e.payload = r.array<uint64_t>(n);
            for (uint32_t id : e.name)
                if (id >= nnames) r.bad = true;
        }
    }
    if (r.bad || r.at != r.b.size() || opt.stage_samples == 0 || T == 0 || S == 0 || mode > 1 || wire > 2) {
        std::fprintf(stderr, "host_parity: malformed scenario %s\n", argv[1]);
        return 2;
    }

    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    Writer w{out};
    std::fwrite("LHDMP001", 1, 8, out);

    int status = 0;
    {
        MetricSystem ms(std::chrono::microseconds(1), false, opt);
        if (npct >= 0) ms.SpecifyPercentiles(pct);
        if (wire) ms.SetWireFormat((WireFormat)wire, keys_in_map);

        std::mutex mu;
        std::condition_variable cv;
        uint32_t open_step = 0; // producers may replay steps < open_step
        uint32_t arrived = 0;   // producers that finished the step being replayed
        std::atomic<bool> create_failed{false};

        auto replay = [&](const Events &e, bool &probed) {
            for (size_t i = 0; i < e.kind.size(); i++) {
                if (e.kind[i] == 1) {
                    ms.Counter(names[e.name[i]], e.payload[i]);
                    continue;
                }
                double v;
                std::memcpy(&v, &e.payload[i], 8);
                ms.Histogram(names[e.name[i]], v);
                if (!probed) { // the engine is created by the first Histogram call
                    probed = true;
                    if (!ms.engine_ready() && ms.last_status() != 4 /* LH_ENODEVICE */) create_failed.store(true);
                }
                if (create_failed.load(std::memory_order_relaxed)) return;
            }
        };
        std::vector<std::thread> producers;
        const uint32_t steps = mode == 0 ? S : 1;
        for (uint32_t t = 0; t < T; t++)
            producers.emplace_back([&, t] {
                bool probed = false;
                for (uint32_t j = 0; j < steps; j++) {
                    {
                        std::unique_lock<std::mutex> g(mu);
                        cv.wait(g, [&] { return open_step > j; });
                    }
                    replay(script[j][t], probed);
                    std::lock_guard<std::mutex> g(mu);
                    arrived++;
                    cv.notify_all();
                }
            });

        std::vector<std::shared_ptr<RawMetricSet>> kept;
        uint32_t seq = 0;
        auto collect = [&](uint32_t step, uint32_t flag) {
            auto raw = ms.collectRawMetrics();
            auto pm = ms.processMetrics(raw);
            ms.addAggregates(raw, *pm);
            dump_interval(w, ms, step, *raw, *pm);
            if (flag == 2) {
                kept.push_back(raw);
            } else {
                raw->Release();
                for (auto &k : kept) k->Release();
                kept.clear();
            }
        };
        for (uint32_t j = 0; j < steps; j++) {
            {
                std::lock_guard<std::mutex> g(mu);
                arrived = 0;
                open_step = j + 1;
            }
            cv.notify_all();
            if (mode == 0) {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return arrived == T; });
                g.unlock();
                if (flags[j] && !create_failed.load()) collect(j, flags[j]);
            } else {
                for (;;) {
                    {
                        std::unique_lock<std::mutex> g(mu);
                        if (cv.wait_for(g, std::chrono::milliseconds(1), [&] { return arrived == T; })) break;
                    }
                    if (!create_failed.load()) collect(seq++, 1);
                }
                if (!create_failed.load()) collect(seq++, 1);
            }
        }
        for (auto &p : producers) p.join();
        for (auto &k : kept) k->Release();
        kept.clear();
        if (create_failed.load()) {
            std::fprintf(stderr, "host_parity: the engine could not be created: status %d\n", ms.last_status());
            status = 3;
        }
        w.put<uint32_t>(2);
        w.put<int32_t>(ms.last_status());
        w.put<uint64_t>(ms.dropped_intervals());
        w.put<uint32_t>(ms.engine_ready() ? 1u : 0u);
    }
    if (std::fclose(out) != 0) { std::perror(argv[2]); return 2; }
    return status;
}
