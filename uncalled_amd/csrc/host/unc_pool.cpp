#include "unc_pool.hpp"

#include <hdf5.h>

#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

namespace unc_host {

// ------------------------------------------------------------------ Paf (read_buffer.cpp:34-160)
static const char *PAF_TAGS[] = {"mt", "wt", "qt", "rt", "ch", "ej", "st", "mx", "tr", "mr", "en", "kp", "dl", "sc", "ce"};

Paf::Paf(const std::string &rd_name, uint16_t channel, uint64_t start_sample) : rd_name_(rd_name) {
    set_int(CHANNEL, channel);
    set_int(READ_START, (int)start_sample);
}

void Paf::set_mapped(uint64_t rd_st, uint64_t rd_en, const std::string &rf_name, uint64_t rf_st, uint64_t rf_en, uint64_t rf_len, bool fwd,
                     uint16_t matches) {
    is_mapped_ = true;
    rd_st_ = rd_st; rd_en_ = rd_en; rf_name_ = rf_name; rf_st_ = rf_st; rf_en_ = rf_en; rf_len_ = rf_len; fwd_ = fwd; matches_ = matches;
}

std::string Paf::str() const {
    std::ostringstream o;
    o << rd_name_ << "\t" << rd_len_ << "\t";
    if (is_mapped_) {
        o << rd_st_ << "\t" << rd_en_ << "\t" << (fwd_ ? '+' : '-') << "\t" << rf_name_ << "\t" << rf_len_ << "\t" << rf_st_ << "\t" << rf_en_
          << "\t" << matches_ << "\t" << (rf_en_ - rf_st_ + 1) << "\t" << 255;
    } else {
        o << "*\t*\t*\t*\t*\t*\t*\t*\t*\t255";
    }
    o << std::fixed;
    for (auto &t : int_tags_) o << "\t" << PAF_TAGS[t.first] << ":i:" << t.second;
    for (auto &t : float_tags_) o << "\t" << PAF_TAGS[t.first] << ":f:" << t.second;
    for (auto &t : str_tags_) o << "\t" << PAF_TAGS[t.first] << ":Z:" << t.second;
    return o.str();
}

void Paf::print_paf() const {
    std::cout << str() << "\n";
    std::cout.flush();
}

// ------------------------------------------------------------------ Fast5Reader (fast5_reader.cpp:62-248) over the HDF5 C API
Fast5Reader::Fast5Reader(const Conf &c)
    : max_reads_(c.max_reads), max_buffer_(c.max_buffer ? c.max_buffer : 100), max_chunks_(c.max_chunks),
      chunk_len_((uint16_t)(c.chunk_time * c.sample_rate)) {
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);   // errors are reported by return values
    if (!c.read_list.empty()) load_read_list(c.read_list);
    if (!c.fast5_list.empty()) load_fast5_list(c.fast5_list);
}

bool Fast5Reader::add_read(const std::string &read_id) {
    if (max_reads_ != 0 && read_filter_.size() >= max_reads_) return false;
    read_filter_.insert(read_id);
    return true;
}

template <class F> static bool each_line(const std::string &fname, const char *what, F take) {
    std::ifstream f(fname);
    if (!f.is_open()) { std::cerr << "Error: failed to open " << what << " list \"" << fname << "\".\n"; return false; }
    std::string line;
    while (std::getline(f, line) && take(line)) {}
    return true;
}
bool Fast5Reader::load_fast5_list(const std::string &fname) {
    return each_line(fname, "fast5", [&](const std::string &l) { if (!l.empty()) add_fast5(l); return true; });
}
bool Fast5Reader::load_read_list(const std::string &fname) {
    return each_line(fname, "read", [&](const std::string &l) { return add_read(l); });
}

bool Fast5Reader::all_buffered() const {
    return (max_reads_ > 0 && total_buffered_ >= max_reads_) || (!read_filter_.empty() && total_buffered_ >= read_filter_.size());
}

bool Fast5Reader::empty() { return buffered_.empty() && read_paths_.empty() && (fast5_list_.empty() || all_buffered()); }

// An HDF5 identifier that closes itself with the H5?close of its kind; move-only (the move constructor deletes copying)
namespace {
class H5 {
public:
    H5(hid_t id, herr_t (*close)(hid_t)) : id_(id), close_(close) {}
    H5(H5 &&o) noexcept : id_(o.id_), close_(o.close_) { o.id_ = -1; }
    ~H5() { if (id_ >= 0) close_(id_); }
    operator hid_t() const { return id_; }
    bool ok() const { return id_ >= 0; }
private:
    hid_t id_;
    herr_t (*close_)(hid_t);
};
H5 string_type(size_t size) {      // a C string type of `size` bytes (or H5T_VARIABLE)
    H5 t(H5Tcopy(H5T_C_S1), H5Tclose);
    H5Tset_size(t, size);
    return t;
}
}  // namespace
static herr_t collect_names(hid_t, const char *name, const H5L_info_t *, void *op) {
    static_cast<std::vector<std::string> *>(op)->push_back(name);
    return 0;
}
static std::vector<std::string> list_group(hid_t f, const std::string &path) {
    std::vector<std::string> names;
    const H5 g(H5Gopen2(f, path.c_str(), H5P_DEFAULT), H5Gclose);
    if (g.ok()) H5Literate(g, H5_INDEX_NAME, H5_ITER_INC, nullptr, collect_names, &names);
    return names;
}
static bool attr_string(hid_t f, const std::string &obj, const char *name, std::string &out) {
    const H5 a(H5Aopen_by_name(f, obj.c_str(), name, H5P_DEFAULT, H5P_DEFAULT), H5Aclose);
    if (!a.ok()) return false;
    const H5 t(H5Aget_type(a), H5Tclose);
    if (H5Tget_class(t) != H5T_STRING) return false;
    if (H5Tis_variable_str(t)) {
        char *p = nullptr;
        if (H5Aread(a, string_type(H5T_VARIABLE), &p) < 0 || !p) return false;
        out = p; free(p);
        return true;
    }
    const size_t n = H5Tget_size(t);
    std::vector<char> buf(n + 1, 0);
    if (H5Aread(a, string_type(n), buf.data()) < 0) return false;
    out = std::string(buf.data(), strnlen(buf.data(), n));
    return true;
}
static bool attr_double(hid_t f, const std::string &obj, const char *name, double &out) {
    const H5 a(H5Aopen_by_name(f, obj.c_str(), name, H5P_DEFAULT, H5P_DEFAULT), H5Aclose);
    if (!a.ok()) return false;
    const H5 t(H5Aget_type(a), H5Tclose);
    if (H5Tget_class(t) == H5T_STRING) {
        std::string s;
        if (!attr_string(f, obj, name, s)) return false;
        out = atof(s.c_str());
        return true;
    }
    if (H5Aread(a, H5T_NATIVE_DOUBLE, &out) < 0) return false;
    if (H5Tget_class(t) == H5T_FLOAT) {
        // ReadBuffer takes every attribute through get_attr_map's strings and atof (read_buffer.cpp:202-222); the fast5
        // library renders a floating attribute with a default-precision stream, i.e. 6 significant digits
        // (range 1534.141357421875 -> "1534.14").  Keep that rounding so the calibrated samples agree.
        std::ostringstream oss;
        oss << out;
        out = atof(oss.str().c_str());
    }
    return true;
}

void Fast5Reader::close_file() { if (file_ >= 0) H5Fclose((hid_t)file_); file_ = -1; }

bool Fast5Reader::open_next() {
    read_paths_.clear();
    close_file();
    if (fast5_list_.empty()) return false;
    const std::string fn = fast5_list_.front();
    fast5_list_.pop_front();
    file_ = (int64_t)H5Fopen(fn.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
    if (file_ < 0) { std::cerr << "Error: failed to open fast5 \"" << fn << "\"\n"; return true; }
    const hid_t f = (hid_t)file_;
    multi_ = true;
    for (const std::string &s : list_group(f, "/")) if (s == "Raw") { multi_ = false; break; }
    for (const std::string &read : list_group(f, multi_ ? "/" : "/Raw/Reads")) {      // multi: the id is in the group's name
        std::string id = read.substr(read.find('_') + 1);
        if (!multi_ && (!attr_string(f, "/Raw/Reads/" + read, "read_id", id) || id.empty())) { std::cerr << "Error: failed to find read_id\n"; return false; }
        if (read_filter_.empty() || read_filter_.count(id)) read_paths_.push_back("/" + read);
    }
    return true;
}

// ReadBuffer(file, raw_path, ch_path), read_buffer.cpp:198-246
bool Fast5Reader::read_one(const std::string &raw_path, const std::string &ch_path, RawRead &r) {
    const hid_t f = (hid_t)file_;
    double v;
    std::string s;
    if (attr_string(f, raw_path, "read_id", s)) r.id = s;
    if (attr_double(f, raw_path, "read_number", v)) r.number = (uint32_t)(int)v;
    if (attr_double(f, raw_path, "start_time", v)) r.start_sample = (uint64_t)(int)v;
    if (attr_string(f, ch_path, "channel_number", s)) r.channel_idx = (uint16_t)(atoi(s.c_str()) - 1);
    else if (attr_double(f, ch_path, "channel_number", v)) r.channel_idx = (uint16_t)((int)v - 1);
    if (attr_double(f, ch_path, "digitisation", v)) r.calib.digitisation = (float)v;      // (a missing one keeps RawRead's 1, 1, 0)
    if (attr_double(f, ch_path, "range", v)) r.calib.range = (float)v;
    if (attr_double(f, ch_path, "offset", v)) r.calib.offset = (float)v;
    const H5 d(H5Dopen2(f, (raw_path + "/Signal").c_str(), H5P_DEFAULT), H5Dclose);
    if (!d.ok()) return false;
    const hssize_t n = H5Sget_simple_extent_npoints(H5(H5Dget_space(d), H5Sclose));
    r.signal.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n <= 0 || H5Dread(d, H5T_NATIVE_INT16, H5S_ALL, H5S_ALL, H5P_DEFAULT, r.signal.data()) >= 0;
    // chunk_count_ > max_chunks: the signal is cut to whole chunks (read_buffer.cpp:229-234)
    if (chunk_len_) {
        const uint64_t cc = r.signal.size() / chunk_len_ + (r.signal.size() % chunk_len_ != 0);
        if (cc > max_chunks_) r.signal.resize((size_t)max_chunks_ * chunk_len_);
    }
    return ok;
}

uint32_t Fast5Reader::fill_buffer() {
    uint32_t count = 0;
    while (buffered_.size() < max_buffer_) {
        if (all_buffered()) { read_paths_.clear(); fast5_list_.clear(); break; }
        while (read_paths_.empty()) if (!open_next()) break;
        if (read_paths_.empty()) break;
        const std::string rp = read_paths_.front();
        const std::string raw_path = multi_ ? rp + "/Raw" : "/Raw/Reads" + rp, ch_path = multi_ ? rp + "/channel_id" : "/UniqueGlobalKey/channel_id";
        read_paths_.pop_front();
        RawRead r;
        if (read_one(raw_path, ch_path, r)) {
            buffered_.push_back(std::move(r));
            count++;
            total_buffered_++;
        }
    }
    return count;
}

RawRead Fast5Reader::pop_read() {
    if (buffered_.empty()) fill_buffer();             // fast5_reader.cpp:236-238
    if (buffered_.empty()) return RawRead();          // exhausted: an empty read (id "", no samples), never UB
    RawRead r = std::move(buffered_.front());
    buffered_.pop_front();
    return r;
}

// ------------------------------------------------------------------ fast5 writer (simulators / tests)
static bool put_attr(hid_t obj, const char *name, hid_t file_t, hid_t mem_t, const void *v) {
    const H5 sp(H5Screate(H5S_SCALAR), H5Sclose);
    const H5 a(H5Acreate2(obj, name, file_t, sp, H5P_DEFAULT, H5P_DEFAULT), H5Aclose);
    return a.ok() && H5Awrite(a, mem_t, v) >= 0;
}
static bool put_attr_str(hid_t obj, const char *name, const std::string &v) {
    const H5 t = string_type(v.size() ? v.size() : 1);
    return put_attr(obj, name, t, t, v.c_str());
}
static bool write_read(hid_t raw_g, hid_t ch_g, const RawRead &r, float sample_rate) {
    const int32_t number = (int32_t)r.number;
    const uint32_t duration = (uint32_t)r.signal.size();
    if (!put_attr_str(raw_g, "read_id", r.id) || !put_attr(raw_g, "read_number", H5T_STD_I32LE, H5T_NATIVE_INT32, &number) ||
        !put_attr(raw_g, "start_time", H5T_STD_U64LE, H5T_NATIVE_UINT64, &r.start_sample) ||
        !put_attr(raw_g, "duration", H5T_STD_U32LE, H5T_NATIVE_UINT32, &duration))
        return false;
    const hsize_t n = r.signal.size();
    const H5 sp(H5Screate_simple(1, &n, nullptr), H5Sclose);
    const H5 d(H5Dcreate2(raw_g, "Signal", H5T_STD_I16LE, sp, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), H5Dclose);
    if (!d.ok() || (n && H5Dwrite(d, H5T_NATIVE_INT16, H5S_ALL, H5S_ALL, H5P_DEFAULT, r.signal.data()) < 0)) return false;
    const double dig = r.calib.digitisation, range = r.calib.range, offset = r.calib.offset, rate = sample_rate;
    return put_attr_str(ch_g, "channel_number", std::to_string(r.channel_idx + 1)) &&
           put_attr(ch_g, "digitisation", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, &dig) && put_attr(ch_g, "range", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, &range) &&
           put_attr(ch_g, "offset", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, &offset) && put_attr(ch_g, "sampling_rate", H5T_IEEE_F64LE, H5T_NATIVE_DOUBLE, &rate);
}

// false when the file, a group, the dataset or an attribute could not be created or written
bool write_fast5(const std::string &path, const std::vector<RawRead> &reads, bool multi, float sample_rate) {
    if (!multi && reads.size() != 1) return false;
    const H5 f(H5Fcreate(path.c_str(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT), H5Fclose);
    if (!f.ok()) return false;
    const H5 lcpl(H5Pcreate(H5P_LINK_CREATE), H5Pclose);
    H5Pset_create_intermediate_group(lcpl, 1);
    for (const RawRead &r : reads) {
        const std::string raw = multi ? "/read_" + r.id + "/Raw" : "/Raw/Reads/Read_" + std::to_string(r.number);
        const std::string ch = multi ? "/read_" + r.id + "/channel_id" : "/UniqueGlobalKey/channel_id";
        const H5 rg(H5Gcreate2(f, raw.c_str(), lcpl, H5P_DEFAULT, H5P_DEFAULT), H5Gclose);
        const H5 cg(H5Gcreate2(f, ch.c_str(), lcpl, H5P_DEFAULT, H5P_DEFAULT), H5Gclose);
        if (!rg.ok() || !cg.ok() || !write_read(rg, cg, r, sample_rate)) return false;
    }
    return true;
}

// Mapper::load_static, mapper.cpp:113-115: a model_path replaces the index's model before anything is made from the index.
// Empty: the compiled-in r9.4 template stays
int index_set_model_path(unc_index_t *ix, const std::string &model_path) {
    if (model_path.empty()) return UNC_OK;
    unc_model_t *m = nullptr;
    if (int rc = unc_model_load(model_path.c_str(), &m)) return rc;
    const int rc = unc_index_set_model(ix, m);
    unc_model_free(m);
    return rc;
}

// ------------------------------------------------------------------ what MapPool and RealtimePool share
void die_last_error() { std::cerr << "Error: " << unc_last_error() << "\n"; abort(); }
unc_index_t *open_index(const Conf &conf, unc_params_t &p) {
    unc_params_default(&p);
    p.max_events = conf.max_events; p.max_chunks = conf.max_chunks;
    p.chunk_time = conf.chunk_time; p.sample_rate = conf.sample_rate;
    unc_index_t *ix = nullptr;
    if (unc_index_load(conf.bwa_prefix.c_str(), conf.idx_preset.c_str(), conf.device, &ix) != UNC_OK ||
        index_set_model_path(ix, conf.model_path) != UNC_OK) die_last_error();
    return ix;
}

Paf paf_from_hit(const unc_index_t *ix, const std::string &id, uint16_t channel_idx, uint64_t start_sample, const unc_hit_t &h) {
    Paf p(id, (uint16_t)(channel_idx + 1), start_sample);
    p.set_read_len(h.rd_len);
    if (h.mapped) p.set_mapped(h.rd_st, h.rd_en, unc_index_seq_name(ix, h.rid), h.rf_st, h.rf_en, h.rf_len, h.fwd != 0, (uint16_t)h.matches);
    if (h.status) std::cerr << "Warning: read " << id << ": device scratch overflow (status " << h.status << "); reported unmapped\n";
    return p;
}
Paf unmapped_paf(const unc_params_t &prms, const std::string &id, uint16_t channel_idx, uint64_t start_sample, uint64_t raw_len) {
    Paf p(id, (uint16_t)(channel_idx + 1), start_sample);
    p.set_read_len((uint64_t)((float)raw_len * (prms.bp_per_sec / prms.sample_rate)));      // bp_per_samp: here only
    return p;
}
std::vector<float> calibrated(const RawRead &r) {
    std::vector<float> out(r.signal.size());
    for (size_t i = 0; i < out.size(); ++i) {
        const float t1 = (float)(int)(uint16_t)r.signal[i] + r.calib.offset;     // (the u16 quirk)
        const float t2 = r.calib.range * t1;
        out[i] = t2 / r.calib.digitisation;
    }
    return out;
}

// ------------------------------------------------------------------ MapPool (map_pool.cpp:28-158), batched on one GPU
MapPool::MapPool(const Conf &conf) : reader_(conf) {
    ix_ = open_index(conf, prms_);
    if (unc_mapper_create(ix_, &prms_, nullptr, &mapper_) != UNC_OK) die_last_error();
    // -t 1 (the reference's default): ONE Mapper maps the reads in input order, and what a read leaves set in sources_added_ is seen
    // by the next (mapper.cpp:88,612-623).  The C ABI reproduces that order exactly (UNC_ORDER_T1: the few reads whose predecessor
    // left flags set are mapped a second time); -t N > 1, where the reference's own outcome depends on which thread gets which
    // read, maps every read independently.
    if (conf.threads <= 1 && unc_mapper_set_read_order(mapper_, UNC_ORDER_T1) != UNC_OK) die_last_error();
    // a batch = four times as many reads as the mapper keeps in flight: every unc_map_batch call ends with the few reads that
    // run to max_events on a nearly idle chip, and at one load of the slots that tail is a third of the call (round 3: 11.5 k
    // reads/s end to end against 17 k in HBM); the FIRST batch is one load of the slots, so that the first PAF lines do not
    // wait for 65 k reads to be read from disk.  --batch-reads overrides; kBatchBytes caps the page-locked memory of a batch.
    uint32_t geo[5] = {0, 0, 0, 0, 0};
    unc_mapper_geometry(mapper_, geo);
    first_batch_reads_ = geo[1] ? geo[1] : 4096;
    batch_reads_ = conf.batch_reads ? conf.batch_reads : 4 * first_batch_reads_;
    if (first_batch_reads_ > batch_reads_) first_batch_reads_ = batch_reads_;
    free_ = {0, 1};
}

MapPool::~MapPool() {
    stop();
    for (Batch &b : bufs_) release(b);
    if (mapper_) unc_mapper_free(mapper_);
    if (ix_) unc_index_free(ix_);
}

void MapPool::add_fast5(const std::string &fname) {
    std::lock_guard<std::mutex> lk(mtx_);
    new_files_.push_back(fname);
    cv_.notify_all();       // an idle loader picks it up
}

void MapPool::release(Batch &b) {
    if (b.raw) { if (b.pinned) unc_host_free(b.raw); else free(b.raw); }
    b.raw = nullptr; b.cap = 0;
}

// Room for `need` samples.  Page-locked memory while the driver hands it out; pageable memory (the C ABI takes either, the
// copy to the device is then staged by the runtime) with one warning when it does not -- a full pinned pool is no reason to
// end a run.
bool MapPool::grow(Batch &b, uint64_t need) {
    if (need <= b.cap) return true;
    uint64_t cap = b.cap ? 2 * b.cap : (32ull << 20);            // at least double, at least what is asked for (in 32 M-sample steps)
    if (cap < need) cap = (need + (32ull << 20) - 1) / (32ull << 20) * (32ull << 20);
    if (cap > kBatchBytes / 2 && need <= kBatchBytes / 2) cap = kBatchBytes / 2;      // never past the byte cap of a batch
    // UNC_STAGING_MAX_KB: a ceiling on one staging buffer for hosts short of (lockable) memory -- and how the tests reach the
    // out-of-memory paths of the loader
    const char *lim_env = getenv("UNC_STAGING_MAX_KB");
    const uint64_t limit = lim_env ? (uint64_t)atoll(lim_env) * 512ull : 0ull;       // in samples
    if (limit) {
        if (need > limit) return false;
        if (cap > limit) cap = limit;
    }
    bool pinned = true;
    int16_t *p = static_cast<int16_t *>(unc_host_alloc(cap * 2));
    if (!p) {
        pinned = false;
        p = static_cast<int16_t *>(malloc(cap * 2));
        if (!p) return false;
        if (!warned_pageable_) {
            std::cerr << "Warning: no page-locked host memory for a staging buffer of " << (cap * 2 >> 20) << " MB: using pageable memory (slower copies)\n";
            warned_pageable_ = true;
        }
    }
    if (b.used) memcpy(p, b.raw, b.used * 2);
    release(b);
    b.raw = p; b.cap = cap; b.pinned = pinned;
    return true;
}

// fast5 files -> staged batches (flattened int16 samples in page-locked memory + per-read offsets / calibration).  Like the
// reference's worker threads (map_pool.cpp:31-42) the two threads live until stop(): files may be added at any time.
void MapPool::loader_main() {
    for (;;) {
        const int bi = claim_buffer();
        if (bi < 0) break;
        Batch &b = bufs_[bi];
        b.reset();
        const uint32_t target = batches_staged_ == 0 ? first_batch_reads_ : batch_reads_;
        std::vector<Paf> unstaged;      // reads no staging buffer could be had for: reported unmapped, like every read the reference is given
        RawRead r;
        while (b.meta.size() < target && !hand_over_early(b) && fetch_read(b, r)) {
            if (stage_read(b, r)) continue;
            // no memory for it: a batch that holds reads is handed over as it is and this read opens the next one; a read that does
            // not even fit an empty buffer gets its unmapped PAF line (every read gets a line, map_pool.cpp:130-158)
            if (!b.meta.empty()) { carry_ = std::move(r); carry_valid_ = true; break; }
            std::cerr << "Error: out of host memory for a staging buffer of " << ((r.signal.size() + 1) * 2 >> 20) << " MB; read " << r.id
                      << " is reported unmapped\n";
            unstaged.push_back(unmapped_paf(prms_, r.id, r.channel_idx, r.start_sample, r.signal.size()));
        }
        if (!publish(bi, unstaged)) break;
    }
}

int MapPool::claim_buffer() {
    std::unique_lock<std::mutex> lk(mtx_);
    cv_.wait(lk, [&] { return stopped_ || !free_.empty(); });
    if (stopped_) return -1;
    const int bi = free_.front();
    free_.pop_front();
    while (!new_files_.empty()) { reader_.add_fast5(new_files_.front()); new_files_.pop_front(); }
    return bi;
}
// the GPU has nothing to do and one load of its slots is staged: batches grow from one load towards four while reading keeps ahead
bool MapPool::hand_over_early(const Batch &b) {
    if (b.meta.size() < first_batch_reads_ || (b.meta.size() & 255u) != 0) return false;
    std::lock_guard<std::mutex> lk(mtx_);
    return !mapper_busy_ && staged_.empty();
}
bool MapPool::fetch_read(const Batch &b, RawRead &r) {
    if (!carry_valid_ && reader_.buffered() == 0 && (reader_.empty() || reader_.fill_buffer() == 0)) return false;
    // (a batch is also closed by bytes: whole reads with -c 1000000 are tens of MB each)
    const uint64_t next_size = carry_valid_ ? carry_.signal.size() : reader_.front_size();
    if (!b.meta.empty() && (b.used + next_size + 1) * 2 > kBatchBytes) return false;
    if (carry_valid_) { r = std::move(carry_); carry_valid_ = false; }      // the read the last batch had no room for
    else r = reader_.pop_read();
    return true;
}

// A buffer that must grow goes straight to what a FULL batch will need: page-locking is slow (seconds for the 4-5 GB of a batch)
// and holds up the mapper thread's HIP calls, so both buffers reach their final size during the first two batches.  But never
// for more reads than are left (UINT32_MAX = unknown): a small input must not page-lock gigabytes it will never fill
uint64_t MapPool::room_wanted(uint64_t used, uint64_t n_staged, uint64_t read_size, uint32_t reads_left, uint32_t batch_reads) {
    const uint64_t least = used + read_size + 1;
    if (n_staged < 16) return least;
    const uint64_t full = reads_left == 0xFFFFFFFFu ? batch_reads : std::min<uint64_t>(batch_reads, n_staged + 1u + reads_left);
    const uint64_t est = (uint64_t)((double)used / (double)n_staged * (double)full * 1.1);
    return std::max(least, std::min(est, kBatchBytes / 2));
}

// Invariant: a read is staged only into a buffer with room for its samples and one more, so a batch that holds reads -- the
// only kind the mapper thread is given -- has cap >= 1 and raw != nullptr even when every read of it is empty (used == 0).
bool MapPool::stage_read(Batch &b, const RawRead &r) {
    const uint64_t least = b.used + r.signal.size() + 1;
    if (least > b.cap && !grow(b, room_wanted(b.used, b.meta.size(), r.signal.size(), reader_.reads_left_if_known(), batch_reads_)) && !grow(b, least))
        return false;
    b.append(r);
    return true;
}
void MapPool::Batch::append(const RawRead &r) {
    if (!r.signal.empty()) memcpy(raw + used, r.signal.data(), r.signal.size() * 2);
    used += r.signal.size();
    off.push_back(used);
    cal.push_back(r.calib);
    meta.push_back(ReadMeta{r.id, r.channel_idx, r.start_sample});
}

bool MapPool::publish(int bi, std::vector<Paf> &unstaged) {
    std::unique_lock<std::mutex> lk(mtx_);
    for (Paf &pf : unstaged) done_.push_back(std::move(pf));
    if (!bufs_[bi].meta.empty()) {
        ++batches_staged_; staged_.push_back(bi);
        cv_.notify_all();
        return true;
    }
    free_.push_front(bi);          // the files ran dry: idle until another one is added
    loader_idle_ = true;
    cv_.notify_all();
    cv_.wait(lk, [&] { return stopped_ || !new_files_.empty(); });
    loader_idle_ = false;
    return !stopped_;
}

void MapPool::mapper_main() {
    for (;;) {
        int bi;
        {
            std::unique_lock<std::mutex> lk(mtx_);
            cv_.wait(lk, [&] { return stopped_ || !staged_.empty(); });
            if (stopped_) break;
            bi = staged_.front();
            staged_.pop_front();
            mapper_busy_ = true;
        }
        Batch &b = bufs_[bi];
        const size_t n = b.meta.size();
        std::vector<unc_hit_t> hits(n);
        if (b.used == 0) b.raw[0] = 0;       // (room for it: the invariant at stage_read)
        const int rc = unc_map_batch(mapper_, (uint32_t)n, b.raw, b.off.data(), b.cal.data(), 0, nullptr, hits.data());
        if (rc != UNC_OK && rc != UNC_ERR_OVERFLOW) die_last_error();
        std::vector<Paf> out;
        out.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            out.push_back(paf_from_hit(ix_, b.meta[i].id, b.meta[i].channel_idx, b.meta[i].start_sample, hits[i]));
            // the read's residence on the device, first event taken up -> result written (the reference times
            // Mapper::map_read on the read's own thread, mapper.cpp:197; here reads share wavefronts in time slices)
            out.back().set_float(Paf::MAP_TIME, hits[i].map_ms);
        }
        std::lock_guard<std::mutex> lk(mtx_);
        for (Paf &p : out) done_.push_back(std::move(p));
        free_.push_back(bi);
        mapper_busy_ = false;
        cv_.notify_all();
    }
}

std::vector<Paf> MapPool::update() {
    std::vector<Paf> ret;
    std::lock_guard<std::mutex> lk(mtx_);
    if (!started_ && !stopped_) {       // the first update starts the pipeline: every add_fast5 of the CLI has happened by then
        started_ = true;
        loader_ = std::thread(&MapPool::loader_main, this);
        mapper_thread_ = std::thread(&MapPool::mapper_main, this);
    }
    ret.swap(done_);
    return ret;
}

bool MapPool::running() {
    std::lock_guard<std::mutex> lk(mtx_);
    if (stopped_) return false;
    if (!started_) return !new_files_.empty() || !reader_.empty();
    // MapPool::running, map_pool.cpp:71-81: files left, a thread at work, or records not yet handed out
    return !(loader_idle_ && new_files_.empty() && staged_.empty() && !mapper_busy_ && done_.empty());
}

void MapPool::stop() {
    {
        std::lock_guard<std::mutex> lk(mtx_);
        stopped_ = true;
        cv_.notify_all();
    }
    if (loader_.joinable()) loader_.join();
    if (mapper_thread_.joinable()) mapper_thread_.join();
}

}  // namespace unc_host
