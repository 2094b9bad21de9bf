// particle_io.hpp — position-only BGEO frames and model sampling for the host drivers.
//
// write_bgeo: the wire format partio emits for the reference's write_partio (Library/MnSystem/IO/ParticleIO.hpp:14-29,
// Externals/partio/io/BGEO.cpp:311-407): Houdini classic BGEO, big-endian: magic 'Bgeo', 'V', version 5, nPoints,
// nPrims 0, nPointGroups 0, nPrimGroups 0, nPointAttrib 0, nVertexAttrib 0, nPrimAttrib 0, nAttrib 0, then per point
// x y z w(=1) as float32, then the two trailing bytes 0x00 0xff.
// With a velocity array (gmpm's opt-in simulation.output_velocity) the frame is what partio writes for a second, VECTOR point attribute
// "v" of 3 floats (BGEO.cpp:345-378): nPointAttrib 1, the attribute's definition behind the header - name as a big-endian 16-bit length and
// its bytes, 16-bit size 3, 32-bit Houdini type 5 (vector), 3 zero defaults - and per point x y z w vx vy vz.
// Further point attributes (gmpm's simulation.output_stress: "stress" of 6 floats, "J", "pressure", "vonmises" of 1) follow the same rule,
// in the order they were added: a FLOAT attribute has Houdini type 0 and as many zero defaults as its size, and every point carries the
// attributes' values behind w in that order.  An INT attribute (gmpm's simulation.output_ids: "id" of 1 int) is partio's INT (BGEO.cpp:360-373,
// :396-400): Houdini type 1, the same 16-bit size and zero defaults, its values big-endian int32 where a FLOAT's float32 stand.
// write_npy_f32: a float32 array as a NumPy .npy file (gmpm's simulation.output_grid).
// write_obj_surface: a triangle soup as a welded Wavefront OBJ file (gmpm's simulation.output_surface).
// read_obj_mesh: its inverse - the vertices and triangles of an OBJ file (gmpm's collision_mesh).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace pio {
using Points = std::vector<std::array<float, 3>>;

inline void put_be32(std::vector<unsigned char>& o, uint32_t v) {
	o.push_back((unsigned char) (v >> 24));
	o.push_back((unsigned char) (v >> 16));
	o.push_back((unsigned char) (v >> 8));
	o.push_back((unsigned char) v);
}
inline void put_bef(std::vector<unsigned char>& o, float f) {
	uint32_t u;
	static_assert(sizeof(u) == sizeof(f), "");
	std::memcpy(&u, &f, 4);
	put_be32(o, u);
}
// A point attribute behind "position": `size` floats a point at data[size * i]; vector: partio's VECTOR (Houdini type 5), else FLOAT (0).
// idata set (data then null): partio's INT (Houdini type 1), `size` int32 a point at idata[size * i].
struct BgeoAttr {
	std::string name;
	int size;
	bool vector;
	const float* data;
	const int32_t* idata = nullptr;
};
inline bool write_bgeo(const std::string& filename, const float* xyz, size_t n, const std::vector<BgeoAttr>& attrs) {
	std::vector<unsigned char> o;
	size_t width = 4;
	for(const BgeoAttr& a: attrs) width += (size_t) a.size;
	o.reserve(256 + n * 4 * width);
	put_be32(o, ((((('B' << 8) | 'g') << 8) | 'e') << 8) | 'o');
	o.push_back('V');
	put_be32(o, 5);
	put_be32(o, (uint32_t) n);// nPoints
	for(int k = 0; k < 3; ++k) put_be32(o, 0);// nPrims, nPointGroups, nPrimGroups
	put_be32(o, (uint32_t) attrs.size());	  // nPointAttrib
	for(int k = 0; k < 3; ++k) put_be32(o, 0);// nVertexAttrib, nPrimAttrib, nAttrib
	for(const BgeoAttr& a: attrs) {
		o.push_back((unsigned char) (a.name.size() >> 8));// name: 16-bit length and its bytes
		o.push_back((unsigned char) a.name.size());
		o.insert(o.end(), a.name.begin(), a.name.end());
		o.push_back((unsigned char) (a.size >> 8));// 16-bit size
		o.push_back((unsigned char) a.size);
		put_be32(o, a.idata ? 1 : a.vector ? 5 : 0);
		for(int k = 0; k < a.size; ++k) put_be32(o, 0);// defaults
	}
	for(size_t i = 0; i < n; ++i) {
		put_bef(o, xyz[3 * i]);
		put_bef(o, xyz[3 * i + 1]);
		put_bef(o, xyz[3 * i + 2]);
		put_bef(o, 1.0f);
		for(const BgeoAttr& a: attrs)
			for(int d = 0; d < a.size; ++d) {
				if(a.idata)
					put_be32(o, (uint32_t) a.idata[(size_t) a.size * i + d]);
				else
					put_bef(o, a.data[(size_t) a.size * i + d]);
			}
	}
	o.push_back(0x00);// "beginExtra" / "endExtra" markers partio appends (BGEO.cpp:424-427)
	o.push_back(0xff);
	std::ofstream f(filename, std::ios::binary);
	if(!f) return false;
	f.write((const char*) o.data(), (std::streamsize) o.size());
	return (bool) f;
}
inline bool write_bgeo(const std::string& filename, const float* xyz, size_t n, const float* vel = nullptr) {
	std::vector<BgeoAttr> attrs;
	if(vel) attrs.push_back({"v", 3, true, vel});
	return write_bgeo(filename, xyz, n, attrs);
}
// The point attributes of gmpm's frames: "v" from vel (may be null), then "stress", "J", "pressure", "vonmises" from stress6 and scalars3
// of mpm_retrieve_stress, here as one array of 9 floats a point {stress6, J, pressure, vonmises} (may be null).  The scalar attributes are
// strided views, so they are copied out first.  Last, "id" from ids (may be null): one INT a point.
inline bool write_bgeo_frame(const std::string& filename, const float* xyz, size_t n, const float* vel, const float* stress9, const int32_t* ids = nullptr) {
	std::vector<BgeoAttr> attrs;
	std::vector<float> s6, sc[3];
	if(vel) attrs.push_back({"v", 3, true, vel});
	if(stress9) {
		s6.resize(6 * n);
		for(auto& v: sc) v.resize(n);
		for(size_t i = 0; i < n; ++i) {
			for(int d = 0; d < 6; ++d) s6[6 * i + d] = stress9[9 * i + d];
			for(int d = 0; d < 3; ++d) sc[d][i] = stress9[9 * i + 6 + d];
		}
		attrs.push_back({"stress", 6, false, s6.data()});
		attrs.push_back({"J", 1, false, sc[0].data()});
		attrs.push_back({"pressure", 1, false, sc[1].data()});
		attrs.push_back({"vonmises", 1, false, sc[2].data()});
	}
	if(ids) attrs.push_back({"id", 1, false, nullptr, ids});
	return write_bgeo(filename, xyz, n, attrs);
}

// A float32 array as a NumPy file (gmpm's simulation.output_grid: the grid volume of mpm_grid_volume beside a frame's BGEO files): format 1.0 -
// the magic "\x93NUMPY", the version bytes 1 0, a little-endian 16-bit header length, the header {'descr': '<f4', 'fortran_order': False,
// 'shape': (d0, d1, ...), } padded with spaces to a newline so that the data starts at a multiple of 64 bytes - then the values in C order
// (last index fastest), little-endian as the host holds them.
inline bool write_npy_f32(const std::string& filename, const float* data, const std::vector<size_t>& shape) {
	std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (";
	size_t count	 = 1;
	for(size_t i = 0; i < shape.size(); ++i) {
		dict += std::to_string(shape[i]) + (i + 1 < shape.size() ? ", " : shape.size() == 1 ? "," : "");
		count *= shape[i];
	}
	dict += "), }";
	const size_t unpadded = 10 + dict.size() + 1;// magic 6, version 2, length 2, the dictionary, the newline
	dict.append((64 - unpadded % 64) % 64, ' ');
	dict += '\n';
	if(dict.size() > 0xffff) return false;
	std::ofstream f(filename, std::ios::binary);
	if(!f) return false;
	const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char) (dict.size() & 0xff), (unsigned char) (dict.size() >> 8)};
	f.write((const char*) head, sizeof(head));
	f.write(dict.data(), (std::streamsize) dict.size());
	static_assert(sizeof(float) == 4, "");
	const uint16_t probe = 1;
	unsigned char first;
	std::memcpy(&first, &probe, 1);
	if(first != 1) return false;// (a big-endian host would have to swap: none of the targets is one)
	if(count) f.write((const char*) data, (std::streamsize) (count * sizeof(float)));
	return (bool) f;
}

// A triangle soup (mpm_grid_isosurface: nine floats a triangle) as a Wavefront OBJ file (gmpm's simulation.output_surface), welded the way
// Engine.isosurface welds: vertices are equal when their position bits are - the surface readout gives triangles that share an edge
// identical bits -, the "v" lines are sorted by those bits (x, then y, then z, as unsigned words), triangles with two equal indices are
// dropped, and the "f" lines keep the soup's order and winding with 1-based indices.  Coordinates are printed with nine significant digits,
// which give the float32 back.
inline bool write_obj_surface(const std::string& filename, const float* tris, size_t ntris) {
	const size_t nv = 3 * ntris;
	std::vector<std::array<uint32_t, 3>> bits(nv);
	if(nv) std::memcpy(bits.data(), tris, nv * 3 * sizeof(float));
	std::vector<uint32_t> order(nv), index(nv);
	for(size_t i = 0; i < nv; ++i) order[i] = (uint32_t) i;
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bits[a] < bits[b]; });
	std::FILE* f = std::fopen(filename.c_str(), "w");
	if(!f) return false;
	uint32_t count = 0;
	for(size_t i = 0; i < nv; ++i) {
		if(i == 0 || bits[order[i]] != bits[order[i - 1]]) {
			++count;
			std::fprintf(f, "v %.9g %.9g %.9g\n", tris[3 * (size_t) order[i]], tris[3 * (size_t) order[i] + 1], tris[3 * (size_t) order[i] + 2]);
		}
		index[order[i]] = count;// 1-based
	}
	for(size_t q = 0; q < ntris; ++q) {
		const uint32_t a = index[3 * q], b = index[3 * q + 1], c = index[3 * q + 2];
		if(a != b && b != c && a != c) std::fprintf(f, "f %u %u %u\n", a, b, c);
	}
	return std::fclose(f) == 0;
}

// The inverse of write_obj_surface, for gmpm's "collision_mesh": the "v x y z" and "f ..." lines of a Wavefront OBJ file as nv x 3 floats and
// nt x 3 zero-based indices.  An "f" entry may carry "/vt/vn" suffixes (ignored), an index may be negative (-1: the last vertex read so
// far), a polygon is fan-triangulated (i0 i1 i2, i0 i2 i3 ...).  Every other line is skipped.  false: the file cannot be read, a "v" or
// "f" line cannot be parsed, or an index points at no vertex read so far.
inline bool read_obj_mesh(const std::string& filename, std::vector<float>& verts, std::vector<int32_t>& tris) {
	verts.clear();
	tris.clear();
	std::ifstream f(filename);
	if(!f) return false;
	std::string line;
	while(std::getline(f, line)) {
		const char* s = line.c_str();
		while(*s == ' ' || *s == '\t') ++s;
		if(s[0] == 'v' && (s[1] == ' ' || s[1] == '\t')) {
			float x[3];
			if(std::sscanf(s + 1, "%f %f %f", &x[0], &x[1], &x[2]) != 3) return false;
			verts.insert(verts.end(), x, x + 3);
		} else if(s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
			std::vector<int32_t> poly;
			const int64_t nv = (int64_t) (verts.size() / 3);
			for(s += 1;;) {
				while(*s == ' ' || *s == '\t' || *s == '\r') ++s;
				if(!*s) break;
				char* end	   = nullptr;
				const long long i = std::strtoll(s, &end, 10);
				if(end == s) return false;
				const int64_t idx = i < 0 ? nv + i : i - 1;
				if(i == 0 || idx < 0 || idx >= nv) return false;
				poly.push_back((int32_t) idx);
				s = end;
				while(*s && *s != ' ' && *s != '\t' && *s != '\r') ++s;// "/vt/vn"
			}
			if(poly.size() < 3) return false;
			for(size_t k = 1; k + 1 < poly.size(); ++k) {
				tris.push_back(poly[0]);
				tris.push_back(poly[k]);
				tris.push_back(poly[k + 1]);
			}
		}
	}
	return true;
}

// The reference's lattice rule (Library/MnBase/Geometry/GeometrySampler.h:11-37): 8 particles per grid node at +-0.25 dx.
template<typename Inside>
inline Points sample_lattice(float dx, const int lo[3], const int hi[3], Inside inside) {
	Points out;
	for(int i = lo[0]; i < hi[0]; ++i)
		for(int j = lo[1]; j < hi[1]; ++j)
			for(int k = lo[2]; k < hi[2]; ++k)
				for(int a = -1; a <= 1; a += 2)
					for(int b = -1; b <= 1; b += 2)
						for(int c = -1; c <= 1; c += 2) {
							std::array<float, 3> p = {(float) (i * dx + a * 0.25 * dx), (float) (j * dx + b * 0.25 * dx), (float) (k * dx + c * 0.25 * dx)};
							if(inside(p)) out.push_back(p);
						}
	return out;
}

// Text level set as read by the reference's SampleGenerator::LoadSDF (Library/MnSystem/IO/PoissonDisk/SampleGenerator.h:68-110):
// "ni nj nk / minx miny minz / dx / phi[ni*nj*nk]" with i fastest.
struct Sdf {
	int n[3]	 = {0, 0, 0};
	float mn[3]	 = {0, 0, 0};
	float dx	 = 0;
	std::vector<float> phi;
	bool load(const std::string& fn) {
		std::ifstream f(fn);
		if(!f) return false;
		f >> n[0] >> n[1] >> n[2] >> mn[0] >> mn[1] >> mn[2] >> dx;
		phi.resize((size_t) n[0] * n[1] * n[2]);
		for(auto& v: phi) f >> v;
		return (bool) f;
	}
	float at(int i, int j, int k) const { return phi[(size_t) i + (size_t) n[0] * ((size_t) j + (size_t) n[1] * k)]; }
	float sample(float x, float y, float z) const {// trilinear, +inf outside
		const float g[3] = {(x - mn[0]) / dx, (y - mn[1]) / dx, (z - mn[2]) / dx};
		int c[3];
		float t[3];
		for(int d = 0; d < 3; ++d) {
			c[d] = (int) std::floor(g[d]);
			t[d] = g[d] - (float) c[d];
			if(c[d] < 0 || c[d] + 1 >= n[d]) return 1e30f;
		}
		float r = 0.f;
		for(int a = 0; a < 2; ++a)
			for(int b = 0; b < 2; ++b)
				for(int e = 0; e < 2; ++e) r += (a ? t[0] : 1 - t[0]) * (b ? t[1] : 1 - t[1]) * (e ? t[2] : 1 - t[2]) * at(c[0] + a, c[1] + b, c[2] + e);
		return r;
	}
};

// Asynchronous output: one worker thread drains a queue of jobs so that the simulation does not wait for the file system
// (the reference's IO singleton, Library/MnSystem/IO/IO.h:10-67: insert_job / flush).  The caller hands over the
// position array by value (moved into the job).
class AsyncWriter {
	std::mutex mut_;
	std::condition_variable cv_, idle_;
	std::deque<std::function<void()>> jobs_;
	bool running_ = true;
	int busy_	  = 0;
	std::thread th_;
	void worker() {
		for(;;) {
			std::function<void()> job;
			{
				std::unique_lock<std::mutex> lk(mut_);
				cv_.wait(lk, [this] { return !running_ || !jobs_.empty(); });
				if(jobs_.empty()) return;// !running_ and drained
				job = std::move(jobs_.front());
				jobs_.pop_front();
				busy_ = 1;
			}
			job();
			{
				std::lock_guard<std::mutex> lk(mut_);
				busy_ = 0;
			}
			idle_.notify_all();
		}
	}

public:
	AsyncWriter()
		: th_([this] { worker(); }) {}
	~AsyncWriter() {
		{
			std::lock_guard<std::mutex> lk(mut_);
			running_ = false;
		}
		cv_.notify_all();
		th_.join();// remaining jobs are written before the thread exits
	}
	void insert_job(std::function<void()> job) {
		{
			std::lock_guard<std::mutex> lk(mut_);
			jobs_.push_back(std::move(job));
		}
		cv_.notify_one();
	}
	void write_bgeo_async(std::string fn, std::vector<float> xyz, size_t n) {
		insert_job([fn = std::move(fn), xyz = std::move(xyz), n] { write_bgeo(fn, xyz.data(), n); });
	}
	void write_bgeo_async(std::string fn, std::vector<float> xyz, std::vector<float> vel, size_t n) {// with the "v" point attribute
		insert_job([fn = std::move(fn), xyz = std::move(xyz), vel = std::move(vel), n] { write_bgeo(fn, xyz.data(), n, vel.data()); });
	}
	void write_bgeo_frame_async(std::string fn, std::vector<float> xyz, std::vector<float> vel, std::vector<float> stress9, size_t n, std::vector<int32_t> ids = {}) {// empty: attribute absent
		insert_job([fn = std::move(fn), xyz = std::move(xyz), vel = std::move(vel), stress9 = std::move(stress9), n, ids = std::move(ids)] {
			write_bgeo_frame(fn, xyz.data(), n, vel.empty() ? nullptr : vel.data(), stress9.empty() ? nullptr : stress9.data(), ids.empty() ? nullptr : ids.data());
		});
	}
	void write_npy_f32_async(std::string fn, std::vector<float> data, std::vector<size_t> shape) {
		insert_job([fn = std::move(fn), data = std::move(data), shape = std::move(shape)] { write_npy_f32(fn, data.data(), shape); });
	}
	void write_obj_surface_async(std::string fn, std::vector<float> tris) {
		insert_job([fn = std::move(fn), tris = std::move(tris)] { write_obj_surface(fn, tris.data(), tris.size() / 9); });
	}
	void flush() {// IO::flush: wait until every queued job has been written
		std::unique_lock<std::mutex> lk(mut_);
		idle_.wait(lk, [this] { return jobs_.empty() && !busy_; });
	}
};
}// namespace pio
