// SdfKit.hpp -- header-only C++ host layer over the C ABI (sdfkit_hip.h) that mirrors the
// reference's public API for the hot path: same type and member names, argument meaning,
// defaults and error behaviour as praeclarum/SdfKit (C#), so that code written against
//   Sdfs / SdfFuncs / SdfExprs / Voxels / MarchingCubes / Mesh
// ports line by line (tests/cpp/reference_suite.cpp restates the reference's NUnit tests).
// The C# shim of INTEGRATION.md is the same layer in the reference's own language; .NET is
// not available in the build image, C++ is.
//
// All compute runs in libsdfkit_hip.so on the GPU.  SDFs are symbolic: arithmetic on
// SdfKit::Val records float32 SSA instructions (the role LINQ expression trees play in the
// reference, GlobalUsings.cs:16), lowered by sdfk_program_create (JIT, like SdfExpr.cs:225-273).
#pragma once
#include <charconv>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "sdfkit_hip.h"

namespace SdfKit {

struct Vector3 {
    float X = 0, Y = 0, Z = 0;
    Vector3() = default;
    Vector3(float x, float y, float z) : X(x), Y(y), Z(z) {}
    explicit Vector3(float v) : X(v), Y(v), Z(v) {}
    static Vector3 One() { return Vector3(1, 1, 1); }
    static Vector3 Zero() { return Vector3(0, 0, 0); }
    float Length() const { return std::sqrt((X * X + Y * Y) + Z * Z); }
};
struct Vector4 {   // (colour, distance) of a sample: what an Sdf delegate writes per point (Sdf.cs:8)
    float X = 0, Y = 0, Z = 0, W = 0;
    Vector4() = default;
    Vector4(float x, float y, float z, float w) : X(x), Y(y), Z(z), W(w) {}
};
inline Vector3 operator+(Vector3 a, Vector3 b) { return {a.X + b.X, a.Y + b.Y, a.Z + b.Z}; }
inline Vector3 operator-(Vector3 a, Vector3 b) { return {a.X - b.X, a.Y - b.Y, a.Z - b.Z}; }
inline Vector3 operator*(Vector3 a, float s) { return {a.X * s, a.Y * s, a.Z * s}; }
inline Vector3 operator*(float s, Vector3 a) { return a * s; }

inline void Check(int status)
{
    if (status != SDFK_OK) throw std::runtime_error(std::string("sdfkit_hip: ") + sdfk_last_error());
}
inline void EnsureInit()
{
    static bool done = false;
    if (!done) {
        Check(sdfk_init(0));
        done = true;
    }
}
// sdfk_set_option / sdfk_get_option (enum sdfk_option): run-time switches that used to be environment variables
inline void SetOption(sdfk_option key, int64_t value) { Check(sdfk_set_option((int32_t)key, value)); }
inline int64_t GetOption(sdfk_option key)
{
    int64_t v = 0;
    Check(sdfk_get_option((int32_t)key, &v));
    return v;
}

// ---------------------------------------------------------------------------------------
// symbolic float32 values (one SSA instruction each)
// ---------------------------------------------------------------------------------------
class Voxels;
struct Builder {
    std::vector<sdfk_op> ops;
    std::vector<const Voxels*> volumes;   // volumes the program reads (sdfk_program_create_bound), slot = index, deduplicated by identity
    int slot(const Voxels* v)
    {
        for (size_t i = 0; i < volumes.size(); i++)
            if (volumes[i] == v) return (int)i;
        if (volumes.size() >= SDFK_MAX_VOLUMES) throw std::logic_error("SdfKit: an SDF program reads at most 8 volumes");
        volumes.push_back(v);
        return (int)volumes.size() - 1;
    }
    int emit(int opcode, int a = -1, int b = -1, int c = -1, int d = -1, float imm = 0.f)
    {
        ops.push_back(sdfk_op{opcode, a, b, c, d, imm});
        return (int)ops.size() - 1;
    }
};

struct Val {
    Builder* b = nullptr;
    int id = -1;
    float k = 0;            // constant payload while not yet bound to a builder
    Val() = default;
    Val(float c) : k(c) {}  // NOLINT: literals convert implicitly, like C# float literals
    Val(Builder* bb, int i) : b(bb), id(i) {}
    int bind(Builder* bb) const { return b ? id : bb->emit(SDFK_OP_CONST, -1, -1, -1, -1, k); }
};
inline Builder* builder_of(const Val& a, const Val& c) { return a.b ? a.b : c.b; }
inline Val bin(int op, const Val& a, const Val& c)
{
    Builder* b = builder_of(a, c);
    if (!b) {   // two literals: the same IEEE binary32 operation, done here
        switch (op) {
        case SDFK_OP_ADD: return Val(a.k + c.k);
        case SDFK_OP_SUB: return Val(a.k - c.k);
        case SDFK_OP_MUL: return Val(a.k * c.k);
        case SDFK_OP_DIV: return Val(a.k / c.k);
        default: throw std::logic_error("SdfKit::Val: this operation needs a symbolic operand");
        }
    }
    const int ia = a.bind(b), ic = c.bind(b);
    return Val(b, b->emit(op, ia, ic));
}
inline Val un(int op, const Val& a)
{
    if (!a.b) {
        switch (op) {
        case SDFK_OP_NEG: return Val(-a.k);
        case SDFK_OP_ABS: return Val(std::fabs(a.k));
        case SDFK_OP_SQRT: return Val(std::sqrt(a.k));
        case SDFK_OP_FLOOR: return Val(std::floor(a.k));
        default: throw std::logic_error("SdfKit::Val: this operation needs a symbolic operand");
        }
    }
    return Val(a.b, a.b->emit(op, a.id));
}
inline Val operator+(const Val& a, const Val& c) { return bin(SDFK_OP_ADD, a, c); }
inline Val operator-(const Val& a, const Val& c) { return bin(SDFK_OP_SUB, a, c); }
inline Val operator*(const Val& a, const Val& c) { return bin(SDFK_OP_MUL, a, c); }
inline Val operator/(const Val& a, const Val& c) { return bin(SDFK_OP_DIV, a, c); }
inline Val operator-(const Val& a) { return un(SDFK_OP_NEG, a); }

struct MathF {   // System.MathF members used by the catalogue
    static Val Sqrt(const Val& a) { return un(SDFK_OP_SQRT, a); }
    static Val Abs(const Val& a) { return un(SDFK_OP_ABS, a); }
    static Val Floor(const Val& a) { return un(SDFK_OP_FLOOR, a); }
    static Val Max(const Val& a, const Val& c) { return bin(SDFK_OP_MAX_IEEE, a, c); }
    static Val Min(const Val& a, const Val& c) { return bin(SDFK_OP_MIN_IEEE, a, c); }
    // The transcendentals of SDF programs (SDFK_OP_SIN .. SDFK_OP_ATAN2: faithful float32 functions, sdfkit_hip.h states them).  They
    // take symbolic values only -- a literal operand alone throws, it would have to be evaluated here -- so that plain float code
    // (IterativeClosestPoint's rotations below) keeps calling the C runtime's std::sin / std::cos and never meets them.
    static Val Sin(const Val& a) { return un(SDFK_OP_SIN, a); }
    static Val Cos(const Val& a) { return un(SDFK_OP_COS, a); }
    static Val Exp(const Val& a) { return un(SDFK_OP_EXP, a); }
    static Val Log(const Val& a) { return un(SDFK_OP_LOG, a); }
    static Val Atan2(const Val& y, const Val& x) { return bin(SDFK_OP_ATAN2, y, x); }   // MathF.Atan2(y, x)
};

struct Vec3 {   // System.Numerics.Vector3 over symbolic components
    Val X, Y, Z;
    Vec3() = default;
    Vec3(Val x, Val y, Val z) : X(x), Y(y), Z(z) {}
    Vec3(Vector3 v) : X(v.X), Y(v.Y), Z(v.Z) {}  // NOLINT
    Val Length() const { return MathF::Sqrt((X * X + Y * Y) + Z * Z); }
    static Vec3 Abs(const Vec3& a) { return {MathF::Abs(a.X), MathF::Abs(a.Y), MathF::Abs(a.Z)}; }
    static Vec3 Max(const Vec3& a, const Vec3& c) { return {bin(SDFK_OP_MAX_SEL, a.X, c.X), bin(SDFK_OP_MAX_SEL, a.Y, c.Y), bin(SDFK_OP_MAX_SEL, a.Z, c.Z)}; }
    static Vec3 Min(const Vec3& a, const Vec3& c) { return {bin(SDFK_OP_MIN_SEL, a.X, c.X), bin(SDFK_OP_MIN_SEL, a.Y, c.Y), bin(SDFK_OP_MIN_SEL, a.Z, c.Z)}; }
    static Val Dot(const Vec3& a, const Vec3& c) { return (a.X * c.X + a.Y * c.Y) + a.Z * c.Z; }
};
inline Vec3 operator+(const Vec3& a, const Vec3& c) { return {a.X + c.X, a.Y + c.Y, a.Z + c.Z}; }
inline Vec3 operator-(const Vec3& a, const Vec3& c) { return {a.X - c.X, a.Y - c.Y, a.Z - c.Z}; }
inline Vec3 operator*(const Val& s, const Vec3& a) { return {s * a.X, s * a.Y, s * a.Z}; }
inline Vec3 operator/(const Vec3& a, const Val& s) { return {a.X / s, a.Y / s, a.Z / s}; }

struct Vec4 {   // SdfOutput = Vector4(colour, distance)
    Val X, Y, Z, W;
    Vec4() = default;
    Vec4(const Vec3& c, Val w) : X(c.X), Y(c.Y), Z(c.Z), W(w) {}
    Vec4(Val x, Val y, Val z, Val w) : X(x), Y(y), Z(z), W(w) {}
};

inline Val Mod(const Val& a, const Val& c) { return a - c * MathF::Floor(a / c); }                       // VectorData.cs:697-698
inline Val VMax(const Vec3& v) { return MathF::Max(MathF::Max(v.X, v.Y), v.Z); }                         // VectorData.cs:860-861
inline Val SelectLt(const Val& a, const Val& c, const Val& t, const Val& f)
{
    Builder* b = a.b ? a.b : (c.b ? c.b : (t.b ? t.b : f.b));
    return Val(b, b->emit(SDFK_OP_SEL_LT, a.bind(b), c.bind(b), t.bind(b), f.bind(b)));
}

// ---------------------------------------------------------------------------------------
// Sdf / SdfFunc
// ---------------------------------------------------------------------------------------
using PointFn = std::function<Vec4(Vec3)>;
using SdfIndexedOutputModifierFunc = std::function<Vec3(Vec3 /*index*/, Vec3 /*position*/, Vec4 /*output*/)>;

class Mesh;
class Voxels;
class MeshSdf;
class DepthFusion;
struct FloatData;
struct Vec3Data;
struct Matrix4x4;

// The reference's `Sdf` delegate (Sdf.cs:8), restricted to SDFs that have a GPU program.
class Sdf {
public:
    Sdf(PointFn fn, bool writesColor) : st_(std::make_shared<State>()) { st_->fn = std::move(fn); st_->writesColor = writesColor; }
    bool WritesColor() const { return st_->writesColor; }
    // the SDF as the flat op list the library compiles (what sdfk_program_create and sdfk_node_* take)
    void Lower(std::vector<sdfk_op>& ops, int32_t out[4], std::vector<const Voxels*>* volumes = nullptr) const
    {
        Builder b;
        Vec3 p(Val(&b, b.emit(SDFK_OP_X)), Val(&b, b.emit(SDFK_OP_Y)), Val(&b, b.emit(SDFK_OP_Z)));
        Vec4 o = st_->fn(p);
        out[0] = out[1] = out[2] = -1;
        out[3] = o.W.bind(&b);
        if (st_->writesColor) { out[0] = o.X.bind(&b); out[1] = o.Y.bind(&b); out[2] = o.Z.bind(&b); }
        ops = b.ops;
        if (volumes) *volumes = b.volumes;
    }
    // A program that reads volumes holds a snapshot of them: an edit of one since (Sample, ClipToBounds, a write through the indexer,
    // MeshSdf::SampleInto) bumps its version, and the next use binds it again.  The Voxels must outlive the Sdf's uses.
    inline sdfk_program* Program() const;
    // SdfEx.WithColor (Sdf.cs:101-115)
    Sdf WithColor(Vector3 color) const { PointFn f = st_->fn; return Sdf([f, color](Vec3 p) { return Vec4(Vec3(color), f(p).W); }, true); }
    Sdf WithColor(float r, float g, float b) const { return WithColor(Vector3(r, g, b)); }
    // SdfEx.Sample (Sdf.cs:22-47): the SDF at arbitrary points; out[i] = (colour, distance) of points[i] -- an SDF that only assigns .W leaves
    // X, Y, Z of the caller's elements alone, like the reference's delegates.  batchSize / maxDegreeOfParallelism have no GPU meaning.
    void Sample(const std::vector<Vector3>& points, std::vector<Vector4>& out, int /*batchSize*/ = 2048, int /*maxDegreeOfParallelism*/ = -1) const
    {
        if (out.size() != points.size()) out.resize(points.size());
        static_assert(sizeof(Vector3) == 12 && sizeof(Vector4) == 16, "plain float triples / quadruples");
        Check(sdfk_eval_points(Program(), points.empty() ? nullptr : &points[0].X, (int64_t)points.size(), out.empty() ? nullptr : &out[0].X));
    }
    // SdfEx.ToVoxels / ToMesh (Sdf.cs:49-63)
    inline Voxels ToVoxels(Vector3 min, Vector3 max, int nx, int ny, int nz, int batchSize = 2048, int maxDegreeOfParallelism = -1, bool clipToBounds = true) const;
    inline Mesh ToMesh(Vector3 min, Vector3 max, int nx, int ny, int nz, int batchSize = 2048, int maxDegreeOfParallelism = -1,
                       bool clipToBounds = true, float isoValue = 0.0f, int step = 1, const std::function<void(float)>& progress = nullptr) const;

private:
    struct State {
        PointFn fn;
        bool writesColor = true;
        sdfk_program* prog = nullptr;
        std::vector<const Voxels*> volumes;
        std::vector<uint64_t> versions;
        ~State() { if (prog) sdfk_program_destroy(prog); }
    };
    std::shared_ptr<State> st_;
};

// per-point SDF (SdfFunc delegate / SdfExpr tree): SdfFuncEx + SdfExprEx members
class SdfFunc {
public:
    SdfFunc(PointFn f) : fn(std::move(f)) {}  // NOLINT
    PointFn fn;
    Sdf ToSdf() const { return Sdf(fn, true); }                                                    // Sdf.cs:301-313, SdfExpr.cs:208-211
    SdfFunc Translate(Vector3 off) const { PointFn f = fn; return SdfFunc([f, off](Vec3 p) { return f(p - Vec3(off)); }); }     // Sdf.cs:315-326
    SdfFunc Translate(float x, float y, float z) const { return Translate(Vector3(x, y, z)); }
    SdfFunc WithColor(Vector3 c) const { PointFn f = fn; return SdfFunc([f, c](Vec3 p) { return Vec4(Vec3(c), f(p).W); }); }    // Sdf.cs:328-340
    SdfFunc WithColor(float r, float g, float b) const { return WithColor(Vector3(r, g, b)); }
    SdfFunc Color(float r, float g, float b) const { return WithColor(r, g, b); }                  // SdfExpr.cs:143-147
    SdfFunc ModifyInput(std::function<Vec3(Vec3)> m) const { PointFn f = fn; return SdfFunc([f, m](Vec3 p) { return f(m(p)); }); }  // SdfExpr.cs:79-89
    static Val Rep(const Val& c, float s) { Val sv(s); return Mod(c + sv * Val(0.5f), sv) - sv * Val(0.5f); }
    static Val Idx(const Val& c, float s) { Val sv(s); return MathF::Floor((c + sv * Val(0.5f)) / sv); }
    SdfFunc RepeatX(float sx) const { return ModifyInput([sx](Vec3 p) { return Vec3(Rep(p.X, sx), p.Y, p.Z); }); }              // SdfExpr.cs:149-153
    SdfFunc RepeatY(float sy) const { return ModifyInput([sy](Vec3 p) { return Vec3(p.X, Rep(p.Y, sy), p.Z); }); }              // SdfExpr.cs:197-201
    SdfFunc RepeatXY(float sx, float sy) const { return ModifyInput([sx, sy](Vec3 p) { return Vec3(Rep(p.X, sx), Rep(p.Y, sy), p.Z); }); }  // SdfExpr.cs:155-161
    SdfFunc RepeatXY(float sx, float sy, SdfIndexedOutputModifierFunc mod) const                  // SdfExpr.cs:163-178
    {
        PointFn f = fn;
        return SdfFunc([f, sx, sy, mod](Vec3 p) {
            Vec3 mp(Rep(p.X, sx), Rep(p.Y, sy), p.Z);
            Vec3 index(Idx(p.X, sx), Idx(p.Y, sy), Val(0.0f));
            Vec4 d = f(mp);
            return Vec4(mod(index, mp, d), d.W);
        });
    }
    SdfFunc RepeatXZ(float sx, float sz, SdfIndexedOutputModifierFunc mod) const                  // SdfExpr.cs:180-195
    {
        PointFn f = fn;
        return SdfFunc([f, sx, sz, mod](Vec3 p) {
            Vec3 mp(Rep(p.X, sx), p.Y, Rep(p.Z, sz));
            Vec3 index(Idx(p.X, sx), Val(0.0f), Idx(p.Z, sz));
            Vec4 d = f(mp);
            return Vec4(mod(index, mp, d), d.W);
        });
    }
};

inline Val BoxDistance(Vec3 p, Vector3 bounds)
{   // Vector3.Max(wd, Zero).Length() + VMax(Vector3.Min(wd, Zero))     Sdf.cs:134-136
    Vec3 wd = Vec3::Abs(p) - Vec3(bounds);
    return Vec3::Max(wd, Vec3(Vector3::Zero())).Length() + VMax(Vec3::Min(wd, Vec3(Vector3::Zero())));
}

struct SdfFuncs {   // Sdf.cs:217-249
    static SdfFunc Box(Vector3 bounds) { return SdfFunc([bounds](Vec3 p) { return Vec4(Vec3(Vector3::One()), BoxDistance(p, bounds)); }); }
    static SdfFunc Box(float b) { return Box(Vector3(b)); }
    static SdfFunc Sphere(float r) { return SdfFunc([r](Vec3 p) { return Vec4(Vec3(Vector3::One()), p.Length() - Val(r)); }); }
    static SdfFunc Union(SdfFunc a, SdfFunc b)
    {
        return SdfFunc([a, b](Vec3 p) {
            Vec4 da = a.fn(p), db = b.fn(p);   // da.W < db.W ? da : db
            return Vec4(SelectLt(da.W, db.W, da.X, db.X), SelectLt(da.W, db.W, da.Y, db.Y), SelectLt(da.W, db.W, da.Z, db.Z), SelectLt(da.W, db.W, da.W, db.W));
        });
    }
};

struct SdfExprs {   // SdfExpr.cs:16-69
    static SdfFunc Box(Vector3 bounds) { return SdfFuncs::Box(bounds); }
    static SdfFunc Box(float b) { return SdfFuncs::Box(b); }
    static SdfFunc Cylinder(float r, float h, Vector3 color = Vector3::One())
    {
        return SdfFunc([r, h, color](Vec3 p) { return Vec4(Vec3(color), MathF::Max(MathF::Sqrt(p.X * p.X + p.Z * p.Z) - Val(r), MathF::Abs(p.Y) - Val(h))); });
    }
    static SdfFunc Solid(std::function<Val(Vec3)> dist, Vector3 color = Vector3::One()) { return SdfFunc([dist, color](Vec3 p) { return Vec4(Vec3(color), dist(p)); }); }
    static SdfFunc Sphere(float r, Vector3 color = Vector3::One()) { return SdfFunc([r, color](Vec3 p) { return Vec4(Vec3(color), p.Length() - Val(r)); }); }
    static SdfFunc Union(SdfFunc a, SdfFunc b) { return SdfFuncs::Union(a, b); }
};

struct Sdfs {   // Sdf.cs:118-215 (batched delegates that only assign .W leave colour zero)
    static Sdf Box(Vector3 bounds) { return Sdf([bounds](Vec3 p) { return Vec4(Val(0.f), Val(0.f), Val(0.f), BoxDistance(p, bounds)); }, false); }
    static Sdf Box(float b) { return Box(Vector3(b)); }
    static Sdf Cylinder(float radius, float height) { return SdfExprs::Cylinder(radius, height).ToSdf(); }
    static Sdf Plane(Vector3 n, float d) { return Sdf([n, d](Vec3 p) { return Vec4(Val(0.f), Val(0.f), Val(0.f), Vec3::Dot(p, Vec3(n)) + Val(d)); }, false); }
    static Sdf PlaneXY(float z = 0) { return Plane(Vector3(0, 0, 1), z); }
    static Sdf PlaneXZ(float y = 0) { return Plane(Vector3(0, 1, 0), y); }
    static Sdf Solid(SdfFunc f) { return Sdf(f.fn, true); }
    static Sdf Solid(std::function<Val(Vec3)> dist, Vector3 color = Vector3::One()) { return Sdf([dist, color](Vec3 p) { return Vec4(Vec3(color), dist(p)); }, true); }
    static Sdf Sphere(float radius) { return Sdf([radius](Vec3 p) { return Vec4(Val(0.f), Val(0.f), Val(0.f), p.Length() - Val(radius)); }, false); }
};

// ---------------------------------------------------------------------------------------
// Mesh (Mesh.cs:8-64)
// ---------------------------------------------------------------------------------------
// MeshSdf::SamplePoints / Mesh::SamplePoints (not in the reference): per sample the point, the unit face normal, the blended colour
// (empty when the mesh has none), the triangle and the barycentric weights of its three vertices as the colour blend used them.
struct MeshSamples {
    std::vector<Vector3> Points, Normals, Colors;
    std::vector<int32_t> Triangles;
    std::vector<Vector3> Weights;
};

// MeshSdf::RayCast / Mesh::RayCast (not in the reference): per ray the first triangle hit (-1: none), the distance in units of
// |direction| (+inf: none) and the barycentric weights of the triangle's three vertices (NaN: none), in MeshSamples' layout.
struct MeshRayHits {
    std::vector<Vector3> Origins, Directions;
    std::vector<int32_t> Triangles;
    std::vector<float> Distances;
    std::vector<Vector3> Weights;
    bool Hit(size_t i) const { return Triangles[i] >= 0; }
    // origin + direction * distance of the hits, in ray order (made on the host)
    std::vector<Vector3> Points() const
    {
        std::vector<Vector3> p;
        for (size_t i = 0; i < Triangles.size(); i++)
            if (Triangles[i] >= 0)
                p.push_back(Vector3(Origins[i].X + Directions[i].X * Distances[i], Origins[i].Y + Directions[i].Y * Distances[i],
                                    Origins[i].Z + Directions[i].Z * Distances[i]));
        return p;
    }
};

// MeshSdf::Components / Mesh::Components (not in the reference): the connected components by index (two vertices with equal
// positions and different indices are different vertices).  Labels are -1 for an unreferenced vertex and an index-degenerate
// triangle; the per-component arrays have Count entries; AreaWeights sums the integer sampling weights of the component's triangles.
struct MeshComponents {
    int64_t Count = 0;
    std::vector<int32_t> VertexLabels, TriangleLabels;
    std::vector<int64_t> Triangles, Vertices, Edges, BoundaryEdges, NonManifoldEdges, OddEdges, InconsistentEdges, AreaWeights;
    int64_t Rounds = 0, ShortcutLaunches = 0;   // what the labels took on the device
    int64_t EulerCharacteristic(size_t c) const { return Vertices[c] - Edges[c] + Triangles[c]; }
    bool IsWatertight(size_t c) const { return OddEdges[c] == 0; }   // (the condition under which ToVoxels' parity sign is well defined)
    bool IsOriented(size_t c) const { return InconsistentEdges[c] == 0 && NonManifoldEdges[c] == 0; }
};

// MeshSdf::Topology / Mesh::Topology: the census of the whole mesh.  Triangles: those that are not index-degenerate; Vertices: referenced.
struct MeshTopology {
    int64_t Components = 0, Triangles = 0, Vertices = 0, Edges = 0, BoundaryEdges = 0, NonManifoldEdges = 0, OddEdges = 0, InconsistentEdges = 0,
            DegenerateTriangles = 0;
    int64_t EulerCharacteristic() const { return Vertices - Edges + Triangles; }
    bool IsWatertight() const { return OddEdges == 0; }
    bool IsOriented() const { return InconsistentEdges == 0 && NonManifoldEdges == 0; }
};

// MeshSdf::Select: the kept vertices' and triangles' old indices, the renumbered index array, the gathered positions and colours.
struct MeshSelection {
    std::vector<int32_t> VertexIndex, TriangleIndex, Triangles;
    std::vector<Vector3> Vertices, Colors;
};

// MeshSdf::Adjacency: the neighbours of vertex v are Neighbors[Start[v] .. Start[v + 1]), ascending, each once (by index;
// index-degenerate triangles connect nothing); Boundary[v] = 1 for the endpoints of an edge with one triangle side.
struct MeshAdjacency {
    std::vector<uint32_t> Start, Neighbors;
    std::vector<uint8_t> Boundary;
    int64_t Degree(size_t v) const { return (int64_t)Start[v + 1] - (int64_t)Start[v]; }
};

// MeshSdf::Weld: VertexMap (one per old vertex: the new index of its representative, -1: dropped), the old indices of the new
// vertices and of the kept triangles, the renumbered index array, the representatives' own positions and colours (zeros when the
// mesh has none), and what went: vertices merged away, triangles dropped as index-degenerate, representatives nothing names, and
// the radix passes the sorts ran.
struct MeshWeld {
    std::vector<int32_t> VertexMap, VertexIndex, TriangleIndex, Triangles;
    std::vector<Vector3> Vertices, Colors;
    int64_t Merged = 0, DegenerateDropped = 0, UnreferencedDropped = 0, Passes = 0;
};

// MeshSdf::Simplify: MeshWeld's fields for the clustered mesh -- VertexMap (one per old vertex: the new number of its group, -1:
// dropped), the representatives' old indices, the kept triangles' old indices, the renumbered index array, the MADE positions and
// colours -- and the triangles dropped for sharing a vertex set with another, and the kept groups whose quadric placement fell
// back to the centroid.
struct MeshSimplify : MeshWeld {
    int64_t DuplicatesDropped = 0, QuadricFallbacks = 0;
};
enum class SimplifyPlacement : int32_t { Representative = SDFK_SIMPLIFY_REPRESENTATIVE, Centroid = SDFK_SIMPLIFY_CENTROID, Quadric = SDFK_SIMPLIFY_QUADRIC };
enum class SimplifyDuplicates : int32_t { One = 0, Keep = SDFK_SIMPLIFY_KEEP_DUPLICATES, Cancel = SDFK_SIMPLIFY_CANCEL_PAIRS };

class Mesh {
public:
    std::vector<Vector3> Vertices, Colors, Normals;
    std::vector<int32_t> Triangles;
    Vector3 Min, Max;
    // A new, smaller Mesh by vertex clustering (MeshSdf::Simplify): the vertices of one cell of the lattice of size cellSize
    // anchored at the origin become one vertex (Quadric: the point nearest the planes of the cell's triangles, kept inside the
    // cell; Centroid: their mean; Representative: the lowest index as it is), and the triangles that collapse or come to lie on
    // top of each other disappear (One: one of each vertex set stays; Keep: all; Cancel: one of an odd number, none of an even
    // one, which keeps a watertight mesh watertight).  Colors come from the call; Normals are recomputed from the new geometry
    // on the side of the representatives' gathered ones (normals = true) or gathered; Min / Max are re-measured; an empty Mesh
    // results when nothing is left.
    inline Mesh Simplify(float cellSize, SimplifyPlacement placement = SimplifyPlacement::Quadric, SimplifyDuplicates duplicates = SimplifyDuplicates::One,
                         bool normals = true) const;
    // A new Mesh with the vertices of equal position made one (MeshSdf::Weld): what a triangle soup, or meshes put together by
    // Concat, need before the members below, which work by index, see their connectivity.  tolerance 0: positions equal as values;
    // tolerance > 0: the vertices of one cell of the lattice of that size anchored at the origin (a lattice, not a ball query).  A
    // group becomes its lowest index, which keeps its own position; Colors and Normals are gathered from the representatives;
    // normals = true recomputes Normals from the welded geometry on the side of the gathered ones.  Min / Max are re-measured;
    // an empty Mesh results when nothing is left.
    inline Mesh Weld(float tolerance = 0.0f, bool normals = false) const;
    // The meshes one after the other, the indices of each offset by the vertices before it (host side; nothing is merged).
    static inline Mesh Concat(const std::vector<Mesh>& meshes);
    // A new Mesh smoothed by `iterations` iterations of Taubin's lambda | mu (MeshSdf::Smooth; mu = 0: plain Laplacian smoothing,
    // which shrinks).  Triangles and Colors are copied; Normals are recomputed from the smoothed positions on the side of the
    // present ones (normals = true) or copied; Min / Max are re-measured.
    inline Mesh Smooth(int iterations = 10, float lambda = 0.5f, float mu = -0.53f, bool pinBoundary = true, bool normals = true) const;
    // A new Mesh whose Normals are made from the geometry (MeshSdf::VertexNormals).  Without an argument the side of the present
    // normals is kept: flipped iff more vertices have a negative dot product with their present normal than a positive one (a
    // tie, or no usable normals, does not flip; marching-cubes meshes wind with their gradient normals and are not flipped).
    inline Mesh RecomputeNormals() const;
    inline Mesh RecomputeNormals(bool flip) const;
    // connectivity by index (MeshSdf(*this).Components / Topology / Select); the Mesh-returning members gather Normals and re-measure
    // Min / Max; a result without components is an empty Mesh
    inline MeshComponents Components() const;
    inline MeshTopology Topology() const;
    inline Mesh SelectComponents(const std::vector<bool>& keep) const;
    // kept iff Triangles >= minTriangles and (double)AreaWeight >= (double)minAreaFraction * (double)total
    inline Mesh RemoveSmallComponents(int64_t minTriangles = 0, float minAreaFraction = 0.0f) const;
    // the greatest AreaWeight; ties: more triangles, then the lower number
    inline Mesh LargestComponent() const;
    // n points on the triangles in proportion to area (MeshSdf(*this).SamplePoints)
    inline MeshSamples SamplePoints(int64_t n, uint64_t seed = 0, bool stratified = true) const;
    // the first hit of every ray, and whether each ray hits anything within the range (MeshSdf(*this).RayCast / Occluded)
    inline MeshRayHits RayCast(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin = 0.0f, float tMax = INFINITY) const;
    inline std::vector<bool> Occluded(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin = 0.0f,
                                      float tMax = INFINITY) const;
    // the generalized winding number of every point, and whether it is inside (MeshSdf(*this).WindingNumber / Contains; beta < 0:
    // the default)
    inline std::vector<float> WindingNumber(const std::vector<Vector3>& points, float beta = -1.0f) const;
    inline std::vector<bool> Contains(const std::vector<Vector3>& points, float beta = -1.0f) const;
    // the mesh rendered as SdfEx.ToImage renders an SDF: the same camera, light, sky and lens (MeshSdf(*this).Render)
    inline Vec3Data ToImage(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees = 60.0f,
                            float nearPlaneDistance = 1.0f, float farPlaneDistance = 100.0f) const;
    inline Vec3Data ToImage(int width, int height, Vector3 cameraPosition, Vector3 cameraTarget, Vector3 cameraUp, float verticalFieldOfViewDegrees = 60.0f,
                            float nearPlaneDistance = 1.0f, float farPlaneDistance = 100.0f) const;
    Vector3 Center() const { return (Min + Max) * 0.5f; }
    Vector3 Size() const { return Max - Min; }
    float Radius() const { return (Max - Min).Length() * 0.5f; }
    // Mesh.WriteObj (Mesh.cs:66-97): `v` lines, then `vn`, then `f a//a b//b c//c`, 1-based
    void WriteObj(std::ostream& w) const
    {
        for (const auto& v : Vertices) w << "v " << FormatSingle(v.X) << ' ' << FormatSingle(v.Y) << ' ' << FormatSingle(v.Z) << '\n';
        for (const auto& v : Normals) w << "vn " << FormatSingle(v.X) << ' ' << FormatSingle(v.Y) << ' ' << FormatSingle(v.Z) << '\n';
        for (size_t i = 0; i + 2 < Triangles.size(); i += 3) {
            const int a = Triangles[i] + 1, b = Triangles[i + 1] + 1, c = Triangles[i + 2] + 1;
            w << "f " << a << "//" << a << ' ' << b << "//" << b << ' ' << c << "//" << c << '\n';
        }
    }
    void WriteObj(const std::string& path) const { std::ofstream f(path); WriteObj(f); }
    // invariant-culture System.Single.ToString() of .NET Core 3.0+ (the runtime global.json pins): shortest round-trip
    // digits through format 'G'; scientific ("d.dddE+XX") when the decimal-point position (decimal exponent + 1) is
    // greater than max(number of digits, 7) or below -3 -- Number.Formatting.cs: nMaxDigits = Math.Max(number.DigitsCount,
    // SinglePrecision), then FormatGeneral's `digPos > nMaxDigits || digPos < -3`.  So 12345678f prints "12345678" (8 digits,
    // position 8), 1e7f prints "1E+07" (1 digit, position 8 > 7), 1e-5f prints "1E-05".
    static std::string FormatSingle(float x)
    {
        if (std::isnan(x)) return "NaN";
        if (std::isinf(x)) return x > 0 ? "Infinity" : "-Infinity";
        if (x == 0) return std::signbit(x) ? "-0" : "0";
        char buf[64];
        auto r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::scientific);   // shortest round-trip: d.ddde±XX
        std::string s(buf, r.ptr);
        const size_t ep = s.find('e');
        std::string mant = s.substr(0, ep);
        const int e = std::stoi(s.substr(ep + 1));
        const bool neg = mant[0] == '-';
        std::string digits;
        for (char c : mant) if (c >= '0' && c <= '9') digits.push_back(c);
        std::string out;
        const int max_digits = (int)std::max<size_t>(digits.size(), 7);
        if (e > -5 && e < max_digits) {
            if (e >= 0) {
                std::string ip = digits.substr(0, std::min(digits.size(), (size_t)e + 1));
                ip.append((size_t)e + 1 - ip.size(), '0');
                const std::string fp = digits.size() > (size_t)e + 1 ? digits.substr(e + 1) : "";
                out = ip + (fp.empty() ? "" : "." + fp);
            } else {
                out = "0." + std::string((size_t)(-e - 1), '0') + digits;
            }
        } else {
            char eb[16];
            snprintf(eb, sizeof eb, "%02d", e < 0 ? -e : e);
            out = digits.substr(0, 1) + (digits.size() > 1 ? "." + digits.substr(1) : "") + "E" + (e >= 0 ? "+" : "-") + eb;
        }
        return neg ? "-" + out : out;
    }
    static Mesh FromHandle(sdfk_mesh* h)
    {
        Mesh m;
        int64_t nv = 0, ni = 0;
        Check(sdfk_mesh_counts(h, &nv, &ni));
        m.Vertices.resize(nv); m.Colors.resize(nv); m.Normals.resize(nv); m.Triangles.resize(ni);
        Check(sdfk_mesh_copy(h, &m.Vertices.data()->X, &m.Colors.data()->X, &m.Normals.data()->X, m.Triangles.data()));
        Check(sdfk_mesh_bounds(h, &m.Min.X, &m.Max.X));
        sdfk_mesh_free(h);
        return m;
    }
};

inline void ReportProgress(const std::function<void(float)>& progress, int nz, int step)
{   // MarchingCubes.cs:53-81: one report per z layer, (float)z / (nz - 2*step)
    if (!progress) return;
    const int zb = nz - 2 * step;
    for (int z = -step; z < zb;) { z += step; progress((float)z / (float)zb); }
}

// ---------------------------------------------------------------------------------------
// Voxels (Voxels.cs)
// ---------------------------------------------------------------------------------------
class Voxels {
public:
    int NX, NY, NZ;
    float DX, DY, DZ;
    Vector3 Min, Max;
    Voxels(Vector3 min, Vector3 max, int nx, int ny, int nz) : NX(nx), NY(ny), NZ(nz), Min(min), Max(max)
    {
        DX = nx >= 1 ? (max.X - min.X) / (float)nx : 0.0f;
        DY = ny >= 1 ? (max.Y - min.Y) / (float)ny : 0.0f;
        DZ = nz >= 1 ? (max.Z - min.Z) / (float)nz : 0.0f;
    }
    Voxels(Voxels&& o) noexcept { *this = std::move(o); }
    Voxels& operator=(Voxels&& o) noexcept
    {
        NX = o.NX; NY = o.NY; NZ = o.NZ; DX = o.DX; DY = o.DY; DZ = o.DZ; Min = o.Min; Max = o.Max; version_ = o.version_ + 1;
        h_ = o.h_; o.h_ = nullptr; hasColors_ = o.hasColors_; values_ = std::move(o.values_); hostNewer_ = o.hostNewer_;
        return *this;
    }
    ~Voxels() { if (h_) sdfk_volume_free(h_); }
    Vector3 Center() const { return (Min + Max) * 0.5f; }
    Vector3 Size() const { return Max - Min; }

    // Voxels.SampleSdf (instance, Voxels.cs:72-125; static, :169-174).  batchSize and
    // maxDegreeOfParallelism are accepted and ignored on the GPU.
    void SampleSdf(const Sdf& sdf, int batchSize = 2048, int maxDegreeOfParallelism = -1) { Sample(sdf, false); }
    static Voxels SampleSdf(const Sdf& sdf, Vector3 min, Vector3 max, int nx, int ny, int nz, int batchSize = 2048, int maxDegreeOfParallelism = -1)
    {
        Voxels v(min, max, nx, ny, nz);
        v.Sample(sdf, false);
        return v;
    }
    void Sample(const Sdf& sdf, bool clip)
    {
        sdfk_program* prog = sdf.Program();
        Ensure(sdf.WritesColor());
        Check(sdfk_sample(prog, h_, clip ? 1 : 0));
        values_.clear();
        hostNewer_ = false;
        version_++;
    }
    void ClipToBounds()   // Voxels.cs:133-167
    {
        Sync();
        Check(sdfk_volume_clip_to_bounds(h_));
        values_.clear();
        version_++;
    }
    // indexer v[ix,iy,iz] (Voxels.cs:42-46): host copy of Values, z fastest
    float& operator()(int ix, int iy, int iz)
    {
        if (values_.empty()) {
            values_.assign((size_t)NX * NY * NZ, 0.0f);
            if (h_) Check(sdfk_volume_download(h_, values_.data(), nullptr));
        }
        hostNewer_ = true;
        version_++;
        return values_[((size_t)ix * NY + iy) * NZ + iz];
    }
    // Inside an SDF (include/sdfkit_hip.h, SDFK_OP_VOXEL_*): the reference's position indexer Voxels[p] (Voxels.cs:48-56; outside the box
    // the nearest boundary voxel instead of IndexOutOfRangeException), the trilinear distance and colour between the cell centres, and
    // the volume as an Sdf (colours when the volume has them, white otherwise).
    Val operator[](const Vec3& p) const { return Read(SDFK_OP_VOXEL_NEAREST, p, 3); }
    Val SampleAt(const Vec3& p) const { return Read(SDFK_OP_VOXEL_LINEAR, p, 3); }
    Vec3 SampleColor(const Vec3& p) const { return Vec3(Read(SDFK_OP_VOXEL_LINEAR, p, 0), Read(SDFK_OP_VOXEL_LINEAR, p, 1), Read(SDFK_OP_VOXEL_LINEAR, p, 2)); }
    Sdf ToSdf(bool interpolate = true) const
    {
        const Voxels* self = this;
        const int op = interpolate ? SDFK_OP_VOXEL_LINEAR : SDFK_OP_VOXEL_NEAREST;
        const bool colored = hasColors_;
        return Sdf([self, op, colored](Vec3 p) {
            const Val w = self->Read(op, p, 3);
            return colored ? Vec4(Vec3(self->Read(op, p, 0), self->Read(op, p, 1), self->Read(op, p, 2)), w) : Vec4(Vec3(Vector3(1.0f, 1.0f, 1.0f)), w);
        }, true);
    }
    uint64_t Version() const { return version_; }
    inline Mesh ToMesh(float isoValue = 0.0f, int step = 1, const std::function<void(float)>& progress = nullptr);
    // A new volume of the same box and shape: the signed distance to this volume's iso-surface with this volume's sign at every
    // voxel, distances beyond maxDistance clamped to +-maxDistance (include/sdfkit_hip.h, "Redistancing").  Colours are copied.
    // stats (optional): sweeps, tile-sweeps, front voxels, clamped voxels.
    Voxels Redistance(float isoValue = 0.0f, float maxDistance = INFINITY, int64_t* stats = nullptr) const
    {
        sdfk_volume* src = const_cast<Voxels*>(this)->Sync();   // (uploads pending host edits: the values stay what they are)
        Voxels out(Min, Max, NX, NY, NZ);
        out.Ensure(hasColors_);
        Check(sdfk_volume_redistance(src, out.h_, isoValue, maxDistance, stats));
        out.version_++;
        return out;
    }
    sdfk_volume* Sync()
    {
        Ensure(hasColors_);
        if (hostNewer_ && !values_.empty()) { Check(sdfk_volume_upload(h_, values_.data(), nullptr)); hostNewer_ = false; }
        return h_;
    }

private:
    friend class MeshSdf;   // (writes distances straight into the device volume)
    friend class KdTree;    // (likewise: KdTree::SampleInto)
    friend class DepthFusion;   // (likewise: DepthFusion::Integrate averages into the device volumes)
    Val Read(int opcode, const Vec3& p, int channel) const
    {
        Builder* b = p.X.b ? p.X.b : (p.Y.b ? p.Y.b : p.Z.b);
        if (!b) throw std::logic_error("SdfKit::Voxels: a volume read needs a symbolic point (inside an SDF)");
        const int x = p.X.bind(b), y = p.Y.bind(b), z = p.Z.bind(b);
        return Val(b, b->emit(opcode, x, y, z, (b->slot(this) << 2) | channel));
    }
    uint64_t version_ = 0;
    void Ensure(bool colors)
    {
        EnsureInit();
        if (h_ && colors && !hasColors_) { sdfk_volume_free(h_); h_ = nullptr; }
        if (!h_) { Check(sdfk_volume_create(NX, NY, NZ, &Min.X, &Max.X, colors ? 1 : 0, &h_)); hasColors_ = colors; }
    }
    sdfk_volume* h_ = nullptr;
    bool hasColors_ = false;
    std::vector<float> values_;
    bool hostNewer_ = false;
};

inline sdfk_program* Sdf::Program() const
{
    if (st_->prog && !st_->volumes.empty()) {
        for (size_t i = 0; i < st_->volumes.size(); i++)
            if (st_->volumes[i]->Version() != st_->versions[i]) { sdfk_program_destroy(st_->prog); st_->prog = nullptr; break; }
    }
    if (!st_->prog) {
        EnsureInit();
        std::vector<sdfk_op> ops;
        int32_t out[4];
        Lower(ops, out, &st_->volumes);
        if (st_->volumes.empty()) {
            Check(sdfk_program_create(ops.data(), (int32_t)ops.size(), out, st_->writesColor ? 1 : 0, &st_->prog));
        } else {
            std::vector<const sdfk_volume*> hs;
            st_->versions.clear();
            for (const Voxels* v : st_->volumes) {
                hs.push_back(const_cast<Voxels*>(v)->Sync());   // (host edits go up first)
                st_->versions.push_back(v->Version());
            }
            Check(sdfk_program_create_bound(ops.data(), (int32_t)ops.size(), out, st_->writesColor ? 1 : 0, hs.data(), (int32_t)hs.size(), &st_->prog));
        }
    }
    return st_->prog;
}

struct MarchingCubes {
    // MarchingCubes.CreateMesh(Voxels, isoValue = 0, step = 1, progress = null)  (MarchingCubes.cs:39)
    static Mesh CreateMesh(Voxels& volume, float isoValue = 0.0f, int step = 1, const std::function<void(float)>& progress = nullptr)
    {
        sdfk_mesh* m = nullptr;
        Check(sdfk_march(volume.Sync(), isoValue, step, &m));
        ReportProgress(progress, volume.NZ, step);
        return Mesh::FromHandle(m);
    }
};

inline Mesh Voxels::ToMesh(float isoValue, int step, const std::function<void(float)>& progress) { return MarchingCubes::CreateMesh(*this, isoValue, step, progress); }

inline Voxels Sdf::ToVoxels(Vector3 min, Vector3 max, int nx, int ny, int nz, int, int, bool clipToBounds) const
{
    Voxels v(min, max, nx, ny, nz);
    v.Sample(*this, clipToBounds);
    return v;
}

inline Mesh Sdf::ToMesh(Vector3 min, Vector3 max, int nx, int ny, int nz, int, int, bool clipToBounds, float isoValue, int step,
                        const std::function<void(float)>& progress) const
{
    EnsureInit();
    sdfk_mesh* m = nullptr;
    Check(sdfk_sample_march(Program(), &min.X, &max.X, nx, ny, nz, clipToBounds ? 1 : 0, isoValue, step, &m));
    ReportProgress(progress, nz, step);
    return Mesh::FromHandle(m);
}

// ---------------------------------------------------------------------------------------
// Node: SdfEx.ToMesh (Sdf.cs:59-63) over several GPUs from THIS process (sdfk_node_*)
// ---------------------------------------------------------------------------------------
// Every listed device gets a context and a rank thread of the library's own; ToMesh fills the caller's four exact-length arrays:
// every GPU copies its own slab into its slice over its own PCIe link (the mesh stays sharded until it is on the host).
class Node {
public:
    explicit Node(const std::vector<int32_t>& devices = {})
    {
        Check(sdfk_node_open(devices.empty() ? nullptr : devices.data(), (int32_t)devices.size(), &h_));
        int32_t backend = 0;
        Check(sdfk_node_info(h_, &world_, &backend));
    }
    ~Node() { if (h_) sdfk_node_close(h_); }
    Node(const Node&) = delete;
    Node& operator=(const Node&) = delete;
    int World() const { return world_; }
    Mesh ToMesh(const Sdf& sdf, Vector3 min, Vector3 max, int nx, int ny, int nz, bool clipToBounds = true, float isoValue = 0.0f) const
    {
        std::vector<sdfk_op> ops;
        int32_t out[4];
        sdf.Lower(ops, out);
        int64_t nv = 0, ni = 0;
        int32_t hasColors = 0;
        Check(sdfk_node_mesh_begin(h_, ops.data(), (int32_t)ops.size(), out, sdf.WritesColor() ? 1 : 0, &min.X, &max.X, nx, ny, nz,
                                   clipToBounds ? 1 : 0, isoValue, &nv, &ni, &hasColors));
        Mesh m;
        m.Vertices.resize(nv); m.Colors.resize(nv); m.Normals.resize(nv); m.Triangles.resize(ni);   // (value-initialised: zero colours already)
        Check(sdfk_node_mesh_copy(h_, nv ? &m.Vertices.data()->X : nullptr, (nv && hasColors) ? &m.Colors.data()->X : nullptr,
                                  nv ? &m.Normals.data()->X : nullptr, ni ? m.Triangles.data() : nullptr, &m.Min.X, &m.Max.X));
        return m;
    }

private:
    sdfk_node* h_ = nullptr;
    int32_t world_ = 1;
};

// ---------------------------------------------------------------------------------------
// RayMarcher (RayMarcher.cs) + the image containers it returns (VectorData.cs)
// ---------------------------------------------------------------------------------------
// The members of System.Numerics.Matrix4x4 the RayMarcher uses, software float32 forms
// (row-major M[r][c] = M(r+1)(c+1)); compile with -ffp-contract=off.
struct Matrix4x4 {
    float M[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    static Vector3 Normalize(Vector3 v) { const float l = std::sqrt((v.X * v.X + v.Y * v.Y) + v.Z * v.Z); return {v.X / l, v.Y / l, v.Z / l}; }
    static Vector3 Cross(Vector3 a, Vector3 b) { return {a.Y * b.Z - a.Z * b.Y, a.Z * b.X - a.X * b.Z, a.X * b.Y - a.Y * b.X}; }
    static float Dot(Vector3 a, Vector3 b) { return (a.X * b.X + a.Y * b.Y) + a.Z * b.Z; }
    static Matrix4x4 CreateLookAt(Vector3 pos, Vector3 target, Vector3 up)
    {
        const Vector3 z = Normalize(pos - target), x = Normalize(Cross(up, z)), y = Cross(z, x);
        Matrix4x4 r;
        const float m[4][4] = {{x.X, y.X, z.X, 0}, {x.Y, y.Y, z.Y, 0}, {x.Z, y.Z, z.Z, 0}, {-Dot(x, pos), -Dot(y, pos), -Dot(z, pos), 1}};
        std::memcpy(r.M, m, sizeof m);
        return r;
    }
    static Matrix4x4 CreatePerspectiveFieldOfView(float fov, float aspect, float nearp, float farp)
    {
        const float ys = 1.0f / std::tan(fov * 0.5f), xs = ys / aspect;
        const float nfr = (std::isinf(farp) && farp > 0) ? -1.0f : farp / (nearp - farp);
        Matrix4x4 r;
        std::memset(r.M, 0, sizeof r.M);
        r.M[0][0] = xs; r.M[1][1] = ys; r.M[2][2] = nfr; r.M[2][3] = -1.0f; r.M[3][2] = nearp * nfr;
        return r;
    }
    friend Matrix4x4 operator*(const Matrix4x4& a, const Matrix4x4& b)
    {
        Matrix4x4 r;
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++)
                r.M[i][j] = ((a.M[i][0] * b.M[0][j] + a.M[i][1] * b.M[1][j]) + a.M[i][2] * b.M[2][j]) + a.M[i][3] * b.M[3][j];
        return r;
    }
    static bool Invert(const Matrix4x4& s, Matrix4x4& out)
    {
        const float a = s.M[0][0], b = s.M[0][1], c = s.M[0][2], d = s.M[0][3], e = s.M[1][0], f = s.M[1][1], g = s.M[1][2], h = s.M[1][3];
        const float i = s.M[2][0], j = s.M[2][1], k = s.M[2][2], l = s.M[2][3], m = s.M[3][0], n = s.M[3][1], o = s.M[3][2], p = s.M[3][3];
        const float kp_lo = k * p - l * o, jp_ln = j * p - l * n, jo_kn = j * o - k * n, ip_lm = i * p - l * m, io_km = i * o - k * m, in_jm = i * n - j * m;
        const float a11 = +(f * kp_lo - g * jp_ln + h * jo_kn), a12 = -(e * kp_lo - g * ip_lm + h * io_km);
        const float a13 = +(e * jp_ln - f * ip_lm + h * in_jm), a14 = -(e * jo_kn - f * io_km + g * in_jm);
        const float det = a * a11 + b * a12 + c * a13 + d * a14;
        if (std::fabs(det) < 1.1920929e-07f) { for (auto& row : out.M) for (float& v : row) v = NAN; return false; }
        const float inv = 1.0f / det;
        float (*R)[4] = out.M;
        R[0][0] = a11 * inv; R[1][0] = a12 * inv; R[2][0] = a13 * inv; R[3][0] = a14 * inv;
        R[0][1] = -(b * kp_lo - c * jp_ln + d * jo_kn) * inv; R[1][1] = +(a * kp_lo - c * ip_lm + d * io_km) * inv;
        R[2][1] = -(a * jp_ln - b * ip_lm + d * in_jm) * inv; R[3][1] = +(a * jo_kn - b * io_km + c * in_jm) * inv;
        const float gp_ho = g * p - h * o, fp_hn = f * p - h * n, fo_gn = f * o - g * n, ep_hm = e * p - h * m, eo_gm = e * o - g * m, en_fm = e * n - f * m;
        R[0][2] = +(b * gp_ho - c * fp_hn + d * fo_gn) * inv; R[1][2] = -(a * gp_ho - c * ep_hm + d * eo_gm) * inv;
        R[2][2] = +(a * fp_hn - b * ep_hm + d * en_fm) * inv; R[3][2] = -(a * fo_gn - b * eo_gm + c * en_fm) * inv;
        const float gl_hk = g * l - h * k, fl_hj = f * l - h * j, fk_gj = f * k - g * j, el_hi = e * l - h * i, ek_gi = e * k - g * i, ej_fi = e * j - f * i;
        R[0][3] = -(b * gl_hk - c * fl_hj + d * fk_gj) * inv; R[1][3] = +(a * gl_hk - c * el_hi + d * ek_gi) * inv;
        R[2][3] = -(a * fl_hj - b * el_hi + d * ej_fi) * inv; R[3][3] = +(a * fk_gj - b * ek_gi + c * ej_fi) * inv;
        return true;
    }
    // (the members IterativeClosestPoint and its tests use; MathF.Sin / Cos are the C runtime's sinf / cosf)
    static Matrix4x4 Identity() { return Matrix4x4(); }
    static Matrix4x4 CreateTranslation(float x, float y, float z)
    {
        Matrix4x4 r;
        r.M[3][0] = x; r.M[3][1] = y; r.M[3][2] = z;
        return r;
    }
    static Matrix4x4 CreateRotationX(float radians)
    {
        const float c = std::cos(radians), s = std::sin(radians);
        Matrix4x4 r;
        r.M[1][1] = c; r.M[1][2] = s; r.M[2][1] = -s; r.M[2][2] = c;
        return r;
    }
    static Matrix4x4 CreateRotationY(float radians)
    {
        const float c = std::cos(radians), s = std::sin(radians);
        Matrix4x4 r;
        r.M[0][0] = c; r.M[0][2] = -s; r.M[2][0] = s; r.M[2][2] = c;
        return r;
    }
    Vector3 Translation() const { return {M[3][0], M[3][1], M[3][2]}; }
    static Vector3 Transform(Vector3 v, const Matrix4x4& m)   // Vector3.Transform(position, matrix)
    {
        return {((v.X * m.M[0][0] + v.Y * m.M[1][0]) + v.Z * m.M[2][0]) + m.M[3][0], ((v.X * m.M[0][1] + v.Y * m.M[1][1]) + v.Z * m.M[2][1]) + m.M[3][1],
                ((v.X * m.M[0][2] + v.Y * m.M[1][2]) + v.Z * m.M[2][2]) + m.M[3][2]};
    }
};

// ---------------------------------------------------------------------------------------
// KdTree (KdTree.cs) and IterativeClosestPoint (IterativeClosestPoint.cs) over sdfk_points_* / sdfk_icp_*
// ---------------------------------------------------------------------------------------
// The search is exact: the static point of least d2, ties to the lowest insertion index (sdfkit_hip.h); SearchKNearest and
// SearchRadius return the k nearest / all within a radius in the same (d2, index) order.  The tree's
// internals (Left, Right, SplitValue, IsLeaf) have no counterpart: the structure is a grid of cell lists on the GPU.
static_assert(sizeof(Vector3) == 3 * sizeof(float), "Vector3 spans are passed as float triples");
class KdTree {
public:
    Vector3 Point;
    const uint8_t SplitAxis;
    explicit KdTree(const std::vector<Vector3>& points, uint8_t axis = 0) : SplitAxis(axis)
    {
        if (points.empty()) throw std::invalid_argument("At least on point must be given (points)");
        EnsureInit();
        Point = points[0];
        Check(sdfk_points_create(reinterpret_cast<const float*>(points.data()), (int64_t)points.size(), &h_));
    }
    KdTree(const KdTree&) = delete;
    KdTree& operator=(const KdTree&) = delete;
    ~KdTree() { sdfk_points_free(h_); }
    int TotalPoints() const
    {
        int64_t n = 0;
        Check(sdfk_points_count(h_, &n));
        return (int)n;
    }
    void AddPoints(const std::vector<Vector3>& points)
    {
        Check(sdfk_points_add(h_, reinterpret_cast<const float*>(points.data()), (int64_t)points.size()));
    }
    Vector3 Search(Vector3 q, float& nearestDistance) const
    {
        Vector3 nearest;
        Check(sdfk_points_search(h_, &q.X, 1, nullptr, &nearestDistance, &nearest.X));
        return nearest;   // (no point counts: the first static point and float.MaxValue, as the reference)
    }
    // Extensions (sdfkit_hip.h, "k nearest / within a radius"): neighbours in (d2, index) order, ascending.
    struct KNearest {
        int K = 0;
        std::vector<int32_t> Indices;   // queries x K; -1 in unused slots
        std::vector<float> Distances;   // queries x K; float.MaxValue in unused slots
        std::vector<int32_t> Found;     // per query: the number of real entries
    };
    struct InRadius {
        std::vector<int64_t> Offsets;   // queries + 1: query i's neighbours are [Offsets[i], Offsets[i + 1])
        std::vector<int32_t> Indices;
        std::vector<float> Distances;
    };
    // the k nearest static points of every query, no farther than maxDistance; 1 <= k <= 64
    KNearest SearchKNearest(const std::vector<Vector3>& queries, int k, float maxDistance = std::numeric_limits<float>::infinity()) const
    {
        KNearest r;
        r.K = k;
        const size_t n = queries.size(), nk = k > 0 ? n * (size_t)k : 0;
        r.Indices.resize(nk);
        r.Distances.resize(nk);
        r.Found.resize(n);
        Check(sdfk_points_knn(h_, reinterpret_cast<const float*>(queries.data()), (int64_t)n, k, maxDistance, r.Indices.data(), r.Distances.data(),
                              r.Found.data()));
        return r;
    }
    // every static point within `radius` of every query (sqrtf(d2) <= radius)
    InRadius SearchRadius(const std::vector<Vector3>& queries, float radius) const
    {
        InRadius r;
        const int64_t n = (int64_t)queries.size();
        const float* q = reinterpret_cast<const float*>(queries.data());
        r.Offsets.assign((size_t)n + 1, 0);
        Check(sdfk_points_radius_count(h_, q, n, radius, r.Offsets.data()));
        r.Indices.resize((size_t)r.Offsets[(size_t)n]);
        r.Distances.resize(r.Indices.size());
        if (!r.Indices.empty()) Check(sdfk_points_radius_fill(h_, q, n, radius, r.Offsets.data(), r.Indices.data(), r.Distances.data()));
        return r;
    }
    // Extensions (sdfkit_hip.h, "Point clouds: normals and volumes").
    struct Normals {
        std::vector<Vector3> Normal;     // per static point; (0, 0, 0) where the neighbourhood is degenerate
        std::vector<float> Variation;    // max(lmin, 0) / (l0 + l1 + l2): never negative, +0 on an exact plane
    };
    // A normal per static point from its k nearest (3 <= k <= 64), turned towards the viewpoints: none (the largest component is
    // made positive -- not a consistent orientation of a closed surface: OrientNormals makes one afterwards), one, or one per point.
    Normals EstimateNormals(int k, const std::vector<Vector3>& viewpoints = {}, float maxDistance = std::numeric_limits<float>::infinity()) const
    {
        Normals r;
        const size_t n = (size_t)TotalPoints();
        r.Normal.resize(n);
        r.Variation.resize(n);
        Check(sdfk_points_normals(h_, k, maxDistance, viewpoints.empty() ? nullptr : &viewpoints[0].X, (int64_t)viewpoints.size(), &r.Normal[0].X,
                                  r.Variation.data()));
        return r;
    }
    Normals EstimateNormals(int k, Vector3 viewpoint, float maxDistance = std::numeric_limits<float>::infinity()) const
    {
        return EstimateNormals(k, std::vector<Vector3>{viewpoint}, maxDistance);
    }
    struct OrientStats { int64_t Rounds = 0, Seeds = 0, Flipped = 0, Unreached = 0, Invalid = 0, Levels[4] = {0, 0, 0, 0}; };
    // `normals` (one per static point) with the sign of some flipped, so that neighbouring normals agree and the top of every connected
    // piece points up: a deterministic region growing over the k-nearest graph (2 <= k <= 64), confident edges first, from at most
    // maxSeeds seeds (sdfkit_hip.h, "Point clouds: a consistent orientation").  Bit-identical to the input up to sign; normals that are
    // not finite or all zero, and those no seed reached, are left alone.
    std::vector<Vector3> OrientNormals(std::vector<Vector3> normals, int k = 8, float maxDistance = std::numeric_limits<float>::infinity(),
                                       int maxSeeds = 64, OrientStats* stats = nullptr) const
    {
        if ((int64_t)normals.size() != (int64_t)TotalPoints()) throw std::invalid_argument("one normal per static point (normals)");
        int64_t st[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        Check(sdfk_points_orient_normals(h_, k, maxDistance, maxSeeds, &normals[0].X, st));
        if (stats) {
            stats->Rounds = st[0]; stats->Seeds = st[1]; stats->Flipped = st[2]; stats->Unreached = st[3]; stats->Invalid = st[4];
            for (int l = 0; l < 4; l++) stats->Levels[l] = st[5 + l];
        }
        return normals;
    }
    // Extension (sdfkit_hip.h, "Point clouds: colours"): the colour at every query from `colors` (one per static point; any three
    // floats -- normals can be averaged the same way): the blend of the k nearest points' colours within maxDistance, weighted as
    // ToVoxels weights their distances; k = 1: the nearest point's colour.  A query with no point within maxDistance: (0, 0, 0), Found 0.
    struct SampledColors {
        std::vector<Vector3> Colors;    // per query
        std::vector<int32_t> Found;     // per query: the neighbours that took part
    };
    SampledColors SampleColors(const std::vector<Vector3>& queries, const std::vector<Vector3>& colors, int k = 8,
                               float maxDistance = std::numeric_limits<float>::infinity()) const
    {
        if ((int64_t)colors.size() != (int64_t)TotalPoints()) throw std::invalid_argument("one colour per static point (colors)");
        SampledColors r;
        r.Colors.resize(queries.size());
        r.Found.resize(queries.size());
        Check(sdfk_points_blend_colors(h_, &colors[0].X, reinterpret_cast<const float*>(queries.data()), (int64_t)queries.size(), k, maxDistance,
                                       reinterpret_cast<float*>(r.Colors.data()), r.Found.data()));
        return r;
    }
    // Extensions (sdfkit_hip.h, "Point clouds: filters").  Neither changes the tree: make a new KdTree from the result.
    struct Downsampled {
        std::vector<Vector3> Points;    // one per occupied voxel, the centroid of its members; voxels in the order of their lowest member
        std::vector<int32_t> Counts;    // the members of each voxel
        std::vector<int32_t> Group;     // per static point: the index of its voxel in Points
        std::vector<Vector3> Colors;    // one per voxel, the mean of its members' colours; empty when no colours were given
    };
    // One point per occupied voxel of the lattice of edge voxelSize anchored at origin.  A voxelSize below the spacing of the cloud
    // returns the points as they are.
    Downsampled VoxelDownsample(float voxelSize, Vector3 origin = Vector3{0.0f, 0.0f, 0.0f}) const
    {
        Downsampled r;
        const size_t n = (size_t)TotalPoints();
        r.Points.resize(n);
        r.Counts.resize(n);
        r.Group.resize(n);
        int64_t m = 0;
        Check(sdfk_points_voxel_downsample(h_, voxelSize, &origin.X, &r.Points[0].X, r.Counts.data(), r.Group.data(), &m));
        r.Points.resize((size_t)m);
        r.Counts.resize((size_t)m);
        return r;
    }
    // ... with one colour per static point (or a normal, or anything else to average): Colors holds every voxel's mean.
    Downsampled VoxelDownsample(float voxelSize, const std::vector<Vector3>& colors, Vector3 origin = Vector3{0.0f, 0.0f, 0.0f}) const
    {
        if ((int64_t)colors.size() != (int64_t)TotalPoints()) throw std::invalid_argument("one colour per static point (colors)");
        Downsampled r;
        const size_t n = (size_t)TotalPoints();
        r.Points.resize(n);
        r.Counts.resize(n);
        r.Group.resize(n);
        r.Colors.resize(n);
        int64_t m = 0;
        Check(sdfk_points_voxel_downsample_colors(h_, voxelSize, &origin.X, &colors[0].X, &r.Points[0].X, r.Counts.data(), r.Group.data(),
                                                  &r.Colors[0].X, &m));
        r.Points.resize((size_t)m);
        r.Counts.resize((size_t)m);
        r.Colors.resize((size_t)m);
        return r;
    }
    struct OutlierStats { int64_t Kept = 0, Removed = 0, Isolated = 0; double Mu = 0, Sigma = 0, Threshold = 0; };
    struct Inliers {
        std::vector<Vector3> Points;        // the kept points, in insertion order
        std::vector<int32_t> Indices;       // their indices, ascending
        std::vector<float> MeanDistance;    // per static point: the mean distance to its k nearest (itself not counted); +inf: isolated
    };
    // The static points whose mean distance to their k nearest (2 <= k <= 64, no farther than maxDistance) is at most
    // mu + stdRatio * sigma over the cloud; a point without a neighbour within maxDistance is isolated and never kept.  The kept
    // points' colours are colors[Indices[i]].  stdRatio: finite and not negative.
    Inliers RemoveStatisticalOutliers(int k, float stdRatio, float maxDistance = std::numeric_limits<float>::infinity(),
                                      OutlierStats* stats = nullptr) const
    {
        Inliers r;
        const size_t n = (size_t)TotalPoints();
        r.Points.resize(n);
        r.Indices.resize(n);
        r.MeanDistance.resize(n);
        int64_t kept = 0, st[6] = {0, 0, 0, 0, 0, 0};
        Check(sdfk_points_outliers(h_, k, stdRatio, maxDistance, r.MeanDistance.data(), nullptr, r.Indices.data(), &r.Points[0].X, &kept, st));
        r.Points.resize((size_t)kept);
        r.Indices.resize((size_t)kept);
        if (stats) {
            stats->Kept = st[0]; stats->Removed = st[1]; stats->Isolated = st[2];
            std::memcpy(&stats->Mu, &st[3], sizeof(double));
            std::memcpy(&stats->Sigma, &st[4], sizeof(double));
            std::memcpy(&stats->Threshold, &st[5], sizeof(double));
        }
        return r;
    }
    struct ClusterStats { int64_t Clusters = 0, Core = 0, Border = 0, Noise = 0, Rounds = 0, Shortcuts = 0; };
    struct Clustered {
        std::vector<int32_t> Labels;     // per static point: its cluster, -1: noise
        std::vector<int32_t> Sizes;      // per cluster: its members, core and border
        std::vector<uint8_t> Core;       // per static point: 1 iff Counts >= minPoints
        std::vector<int32_t> Counts;     // per static point: the static points within the radius, itself and its duplicates included
    };
    struct Selected {
        std::vector<Vector3> Points;     // the kept points, in insertion order
        std::vector<int32_t> Indices;    // their indices, ascending
        std::vector<int32_t> Labels;     // RemoveSmallClusters only: Clusters' labels of all static points
    };
    // Density clustering of the static points (DBSCAN; minPoints = 1: Euclidean cluster extraction): a point is core iff at least
    // minPoints static points lie within the radius (sqrtf(d2) <= radius, itself included); clusters are the connected components
    // of the core points, numbered by their lowest core member; any other point takes the cluster of the core point within the radius
    // that is first in (d2, index) order, or is noise (-1).  The result depends on no order.
    Clustered Clusters(float radius, int minPoints = 1, ClusterStats* stats = nullptr) const
    {
        Clustered r;
        const size_t n = (size_t)TotalPoints();
        r.Labels.resize(n);
        r.Sizes.resize(n);
        r.Core.resize(n);
        r.Counts.resize(n);
        int64_t c = 0, st[6] = {0, 0, 0, 0, 0, 0};
        Check(sdfk_points_cluster(h_, radius, minPoints, r.Labels.data(), r.Sizes.data(), r.Core.data(), r.Counts.data(), &c, st));
        r.Sizes.resize((size_t)c);
        if (stats) *stats = ClusterStats{st[0], st[1], st[2], st[3], st[4], st[5]};
        return r;
    }
    // The static points whose cluster is kept: 0 <= label < keep.size() and keep[label] != 0.  labels: one per static point,
    // Clusters' or any other.
    Selected SelectClusters(const std::vector<int32_t>& labels, const std::vector<uint8_t>& keep) const
    {
        if ((int64_t)labels.size() != (int64_t)TotalPoints()) throw std::invalid_argument("one label per static point (labels)");
        Selected r;
        const size_t n = labels.size();
        r.Points.resize(n);
        r.Indices.resize(n);
        int64_t kept = 0;
        Check(sdfk_points_select(h_, labels.data(), keep.empty() ? nullptr : keep.data(), (int64_t)keep.size(), r.Indices.data(), &r.Points[0].X, &kept));
        r.Points.resize((size_t)kept);
        r.Indices.resize((size_t)kept);
        return r;
    }
    // Clusters, then the points of the clusters of at least minSize members; noise goes.
    Selected RemoveSmallClusters(float radius, int minPoints = 1, int minSize = 2, ClusterStats* stats = nullptr) const
    {
        Clustered c = Clusters(radius, minPoints, stats);
        std::vector<uint8_t> keep(c.Sizes.size());
        for (size_t i = 0; i < keep.size(); i++) keep[i] = c.Sizes[i] >= minSize ? 1 : 0;
        Selected r = SelectClusters(c.Labels, keep);
        r.Labels = std::move(c.Labels);
        return r;
    }
    // Clusters, then the points of the cluster of greatest size (ties: the lowest number); nothing without a cluster.
    Selected LargestCluster(float radius, int minPoints = 1) const
    {
        const Clustered c = Clusters(radius, minPoints);
        std::vector<uint8_t> keep(c.Sizes.size(), 0);
        size_t best = 0;
        for (size_t i = 1; i < keep.size(); i++)
            if (c.Sizes[i] > c.Sizes[best]) best = i;
        if (!keep.empty()) keep[best] = 1;
        return SelectClusters(c.Labels, keep);
    }
    struct VolumeStats { int64_t Known = 0, Unknown = 0, Candidates = 0, Queries = 0; };
    // The cloud with one outward normal per static point as a signed distance volume: the blend of the tangent-plane distances of the
    // k nearest points within maxDistance; voxels beyond get +-maxDistance (give a band, then Voxels::Redistance, for a full field).
    Voxels ToVoxels(const std::vector<Vector3>& normals, Vector3 min, Vector3 max, int nx, int ny, int nz, int k = 8,
                    float maxDistance = std::numeric_limits<float>::infinity(), bool clipToBounds = false, VolumeStats* stats = nullptr) const
    {
        Voxels v(min, max, nx, ny, nz);
        SampleInto(v, normals, k, maxDistance, stats);
        if (clipToBounds) v.ClipToBounds();
        return v;
    }
    // ... with one colour per static point: the volume's colours are SampleColors at every cell centre (zero where no point lies
    // within maxDistance), which Redistance copies and ToMesh interpolates onto the vertices.
    Voxels ToVoxels(const std::vector<Vector3>& normals, const std::vector<Vector3>& colors, Vector3 min, Vector3 max, int nx, int ny, int nz,
                    int k = 8, float maxDistance = std::numeric_limits<float>::infinity(), bool clipToBounds = false,
                    VolumeStats* stats = nullptr) const
    {
        Voxels v(min, max, nx, ny, nz);
        SampleInto(v, normals, k, maxDistance, stats, &colors);
        if (clipToBounds) v.ClipToBounds();
        return v;
    }
    // colors: null leaves the volume's colours alone; otherwise they are overwritten (a volume without colour storage gets it)
    void SampleInto(Voxels& v, const std::vector<Vector3>& normals, int k = 8, float maxDistance = std::numeric_limits<float>::infinity(),
                    VolumeStats* stats = nullptr, const std::vector<Vector3>* colors = nullptr) const
    {
        if ((int64_t)normals.size() != (int64_t)TotalPoints()) throw std::invalid_argument("one normal per static point (normals)");
        if (colors && (int64_t)colors->size() != (int64_t)TotalPoints()) throw std::invalid_argument("one colour per static point (colors)");
        if (colors) v.Ensure(true);   // (a device copy without colour storage is dropped: every voxel of it is written below)
        if (v.hostNewer_) v.Sync(); else v.Ensure(v.hasColors_);   // (host edits go up first; the colours stay what they are)
        int64_t st[4] = {0, 0, 0, 0};
        if (colors) Check(sdfk_points_to_volume_colors(h_, &normals[0].X, &(*colors)[0].X, v.h_, k, maxDistance, stats ? st : nullptr));
        else Check(sdfk_points_to_volume(h_, &normals[0].X, v.h_, k, maxDistance, stats ? st : nullptr));
        if (stats) { stats->Known = st[0]; stats->Unknown = st[1]; stats->Candidates = st[2]; stats->Queries = st[3]; }
        v.values_.clear();
        v.hostNewer_ = false;
        v.version_++;
    }
    sdfk_points* Handle() const { return h_; }

private:
    sdfk_points* h_ = nullptr;
};

class IterativeClosestPoint {
public:
    int MaxIterations = 100;
    float GoodCorrespondenceDistance = 0.01f;
    float ConvergedMaximumTranslation = 1.0e-4f;
    float ConvergedMaximumRotation = 1.0e-5f;
    int Iterations = 0;   // (extension: iterations of the last RegisterPoints)

    explicit IterativeClosestPoint(const std::vector<Vector3>& staticPoints) : tree_(new KdTree(staticPoints)) {}
    explicit IterativeClosestPoint(const std::vector<std::vector<Vector3>>& staticPoints)
    {
        if (staticPoints.empty()) throw std::invalid_argument("At least one set of points must be given (staticPoints)");
        tree_.reset(new KdTree(staticPoints[0]));
        for (size_t i = 1; i < staticPoints.size(); i++) tree_->AddPoints(staticPoints[i]);
    }
    // Extension (sdfkit_hip.h, "point to plane"): one normal per static point, e.g. StaticTree().EstimateNormals(k).Normal.  With normals
    // set, RegisterPoints minimises the distances to the tangent planes at the nearest static points; their orientation does not
    // matter, and a point whose normal is (0, 0, 0) takes no part.
    enum class Metric { Auto, Point, Plane };   // Auto: Plane iff normals are set
    struct PlaneStats {
        bool Valid = false;        // false after a point-to-point registration
        int64_t Kept = 0;          // kept correspondences of the last iteration
        double SumR2 = 0.0;        // sum of their squared plane distances before the step
        bool Converged = false;
        int Retained = 0;          // eigenvalues of the normal equations the solve retained (6: every direction observed)
    };
    PlaneStats LastStats;
    bool HasStaticNormals() const { return hasNormals_; }
    const std::vector<Vector3>& StaticNormals() const { return normals_; }
    void SetStaticNormals(const std::vector<Vector3>& normals)
    {
        if ((int64_t)normals.size() != (int64_t)tree_->TotalPoints()) throw std::invalid_argument("one normal per static point (StaticNormals)");
        normals_ = normals;
        hasNormals_ = true;
    }
    void ClearStaticNormals() { normals_.clear(); hasNormals_ = false; }
    KdTree& StaticTree() { return *tree_; }

    void AddStaticPoints(const std::vector<Vector3>& staticPoints)
    {
        if (hasNormals_) throw std::invalid_argument("AddStaticPoints would leave StaticNormals out of step: pass the new points' normals");
        tree_->AddPoints(staticPoints);
    }
    void AddStaticPoints(const std::vector<Vector3>& staticPoints, const std::vector<Vector3>& normals)
    {
        if (!hasNormals_) throw std::invalid_argument("AddStaticPoints with normals: set StaticNormals first");
        if (normals.size() != staticPoints.size()) throw std::invalid_argument("one normal per added point (normals)");
        tree_->AddPoints(staticPoints);
        normals_.insert(normals_.end(), normals.begin(), normals.end());
    }
    // Rigidly moves `points` (in place) onto the static points; returns the transform that did it.
    Matrix4x4 RegisterPoints(std::vector<Vector3>& points, Metric metric = Metric::Auto)
    {
        const sdfk_icp_params prm{MaxIterations, GoodCorrespondenceDistance, ConvergedMaximumTranslation, ConvergedMaximumRotation};
        Matrix4x4 total;
        int32_t iters = 0;
        if (metric == Metric::Plane && !hasNormals_) throw std::invalid_argument("Metric::Plane needs StaticNormals");
        LastStats = PlaneStats();
        if (metric == Metric::Plane || (metric == Metric::Auto && hasNormals_)) {
            if ((int64_t)normals_.size() != (int64_t)tree_->TotalPoints()) throw std::invalid_argument("StaticNormals is out of step with the static points");
            int64_t st[4] = {0, 0, 0, 0};
            Check(sdfk_icp_register_plane(tree_->Handle(), &prm, reinterpret_cast<const float*>(normals_.data()), reinterpret_cast<float*>(points.data()),
                                          (int64_t)points.size(), &total.M[0][0], &iters, st));
            LastStats.Valid = true;
            LastStats.Kept = st[0];
            std::memcpy(&LastStats.SumR2, &st[1], sizeof(double));
            LastStats.Converged = st[2] != 0;
            LastStats.Retained = (int)st[3];
        } else {
            Check(sdfk_icp_register(tree_->Handle(), &prm, reinterpret_cast<float*>(points.data()), (int64_t)points.size(), &total.M[0][0], &iters));
        }
        Iterations = iters;
        return total;
    }
    std::vector<Matrix4x4> GlobalRegisterPoints(const std::vector<std::vector<Vector3>>& staticPoints, std::vector<std::vector<Vector3>>& dynamicPoints)
    {
        if (dynamicPoints.empty()) return {};
        IterativeClosestPoint icp(staticPoints);
        std::vector<Matrix4x4> transforms;
        for (auto& d : dynamicPoints) {
            transforms.push_back(icp.RegisterPoints(d));
            icp.AddStaticPoints(d);
        }
        return transforms;
    }
    std::vector<Matrix4x4> GlobalRegisterPoints(std::vector<std::vector<Vector3>>& points)
    {
        if (points.empty()) return {};
        if (points.size() == 1) return {Matrix4x4::Identity()};
        std::vector<std::vector<Vector3>> s(points.begin(), points.begin() + 1), d(points.begin() + 1, points.end());
        auto r = GlobalRegisterPoints(s, d);
        for (size_t i = 0; i < d.size(); i++) points[i + 1] = d[i];
        return r;
    }

private:
    std::unique_ptr<KdTree> tree_;
    std::vector<Vector3> normals_;
    bool hasNormals_ = false;
};

inline void WriteTgaHeader(std::ostream& w, int imageType, int width, int height, int bpp)
{   // VectorData.cs:246-261: 18-byte header, top-down
    const unsigned char h[18] = {0, 0, (unsigned char)imageType, 0, 0, 0, 0, 0, 0, 0, 0, 0, (unsigned char)(width & 255), (unsigned char)(width >> 8),
                                 (unsigned char)(height & 255), (unsigned char)(height >> 8), (unsigned char)bpp, 0x20};
    w.write(reinterpret_cast<const char*>(h), 18);
}
// ---------------------------------------------------------------------------------------
// Triangle meshes as signed distance fields (not in the reference: Mesh -> Voxels), sdfk_trimesh_* (include/sdfkit_hip.h)
// ---------------------------------------------------------------------------------------
enum class MeshSign : int32_t { Parity = SDFK_TRIMESH_SIGN_PARITY, Winding = SDFK_TRIMESH_SIGN_WINDING };
// the smallest beta of the recorded list at which every case of tests/golden/mesh_winding_accuracy.json keeps every sign
constexpr float DefaultWindingBeta = 2.5f;

class MeshSdf {
public:
    // The triangles of `vertices` / `triangles` (three indices each); `colors` (one per vertex) may be empty.
    MeshSdf(const std::vector<Vector3>& vertices, const std::vector<int32_t>& triangles, const std::vector<Vector3>& colors = {})
    {
        EnsureInit();
        hasColors_ = !colors.empty();
        if (hasColors_ && colors.size() != vertices.size()) throw std::invalid_argument("one colour per vertex (colors)");
        Check(sdfk_trimesh_create(reinterpret_cast<const float*>(vertices.data()), (int64_t)vertices.size(), triangles.data(),
                                  (int64_t)triangles.size(), hasColors_ ? reinterpret_cast<const float*>(colors.data()) : nullptr, &h_));
        nv_ = (int64_t)vertices.size();
        nt_ = (int64_t)triangles.size() / 3;
    }
    explicit MeshSdf(const Mesh& m) : MeshSdf(m.Vertices, m.Triangles, AnyNonZero(m.Colors) ? m.Colors : std::vector<Vector3>{}) {}
    MeshSdf(const MeshSdf&) = delete;
    MeshSdf& operator=(const MeshSdf&) = delete;
    ~MeshSdf() { sdfk_trimesh_free(h_); }
    // Every query at once: the nearest triangle (-1 for a NaN / infinite query), its f32 distance and closest point.
    void Search(const std::vector<Vector3>& queries, std::vector<int32_t>& triangle, std::vector<float>& distance, std::vector<Vector3>& closest) const
    {
        triangle.resize(queries.size()); distance.resize(queries.size()); closest.resize(queries.size());
        if (queries.empty()) return;
        Check(sdfk_trimesh_closest(h_, &queries.data()->X, (int64_t)queries.size(), triangle.data(), distance.data(), &closest.data()->X));
    }
    // The signed distance at the cell centres of Voxels(min, max, nx, ny, nz); distances above maxDistance become
    // +-maxDistance.  Without a band, large volumes far from a fine mesh are slow.
    // sign: MeshSign::Parity (crossings along z: exact on watertight meshes, streaks on others) or MeshSign::Winding
    // (|WindingNumber| > 1/2 with the acceptance parameter beta: holes are capped by the 1/2 level set and overlapping pieces are
    // united; the values next to a cap are distances to the mesh's triangles, not to the cap, until Voxels::Redistance has run).
    Voxels ToVoxels(Vector3 min, Vector3 max, int nx, int ny, int nz, float maxDistance = INFINITY, bool clipToBounds = false,
                    MeshSign sign = MeshSign::Parity, float beta = DefaultWindingBeta) const
    {
        Voxels v(min, max, nx, ny, nz);
        SampleInto(v, maxDistance, sign, beta);
        if (clipToBounds) v.ClipToBounds();
        return v;
    }
    void SampleInto(Voxels& v, float maxDistance = INFINITY, MeshSign sign = MeshSign::Parity, float beta = DefaultWindingBeta) const
    {
        v.Ensure(hasColors_ || v.hasColors_);
        if (sign == MeshSign::Parity) Check(sdfk_trimesh_to_volume(h_, v.h_, maxDistance));
        else Check(sdfk_trimesh_to_volume_signed(h_, v.h_, maxDistance, (int32_t)sign, beta));
        v.values_.clear();
        v.hostNewer_ = false;
        v.version_++;
    }
    // n points on the triangles in proportion to area (sdfk_trimesh_sample: one stated function of the mesh, n, seed and the mode).
    // stratified: one sample per equal share of the total area, in triangle order; otherwise independent draws.  Normals: the unit
    // face normals of the winding (b - a) x (c - a).  A mesh in which no triangle has an area is refused.
    MeshSamples SamplePoints(int64_t n, uint64_t seed = 0, bool stratified = true) const
    {
        MeshSamples s;
        const int32_t flags = stratified ? SDFK_TRIMESH_SAMPLE_STRATIFIED : 0;
        if (n < 0 || n >= (int64_t(1) << 31))   // (the library refuses it: nothing is allocated for it first)
            Check(sdfk_trimesh_sample(h_, n, seed, flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        const size_t m = n > 0 ? (size_t)n : 0;
        s.Points.resize(m); s.Normals.resize(m); s.Triangles.resize(m); s.Weights.resize(m);
        if (hasColors_) s.Colors.resize(m);
        Check(sdfk_trimesh_sample(h_, n, seed, flags, &s.Points.data()->X, &s.Normals.data()->X,
                                  hasColors_ ? &s.Colors.data()->X : nullptr, s.Triangles.data(), &s.Weights.data()->X, sampleStats_));
        return s;
    }
    // The connected components by index with a row of counts each (sdfk_trimesh_components, sdfk_trimesh_topology).
    MeshComponents Components() const
    {
        MeshComponents c;
        int64_t nv = 0, nt = 0, stats[4] = {0, 0, 0, 0}, census[8];
        Counts(&nv, &nt);
        c.VertexLabels.resize((size_t)nv); c.TriangleLabels.resize((size_t)nt);
        Check(sdfk_trimesh_components(h_, c.VertexLabels.data(), c.TriangleLabels.data(), &c.Count, stats));
        std::vector<int64_t> rows((size_t)c.Count * 8);
        Check(sdfk_trimesh_topology(h_, census, rows.data(), c.Count));
        std::vector<int64_t>* cols[8] = {&c.Triangles, &c.Vertices, &c.Edges, &c.BoundaryEdges, &c.NonManifoldEdges, &c.OddEdges, &c.InconsistentEdges,
                                         &c.AreaWeights};
        for (int k = 0; k < 8; k++) {
            cols[k]->resize((size_t)c.Count);
            for (size_t i = 0; i < (size_t)c.Count; i++) (*cols[k])[i] = rows[8 * i + k];
        }
        c.Rounds = stats[0]; c.ShortcutLaunches = stats[1];
        return c;
    }
    // The edge census of the whole mesh (sdfk_trimesh_topology).
    MeshTopology Topology() const
    {
        int64_t census[8], nv = 0, nt = 0;
        Counts(&nv, &nt);
        Check(sdfk_trimesh_topology(h_, census, nullptr, 0));
        MeshTopology t;
        t.Components = census[0]; t.Vertices = census[1]; t.Edges = census[2]; t.BoundaryEdges = census[3]; t.NonManifoldEdges = census[4];
        t.OddEdges = census[5]; t.InconsistentEdges = census[6]; t.DegenerateTriangles = census[7];
        t.Triangles = nt - census[7];
        return t;
    }
    // The sub-mesh of the components whose flag is set (sdfk_trimesh_select): one flag per component.
    MeshSelection Select(const std::vector<bool>& keep) const
    {
        int64_t nv = 0, nt = 0, count = 0, kv = 0, kt = 0;
        Counts(&nv, &nt);
        Check(sdfk_trimesh_components(h_, nullptr, nullptr, &count, nullptr));
        if ((int64_t)keep.size() != count) throw std::invalid_argument("one flag per component (keep)");
        std::vector<uint8_t> k(keep.size() + 1, 0);   // (never empty: a NULL keep array is refused)
        for (size_t i = 0; i < keep.size(); i++) k[i] = keep[i] ? 1 : 0;
        MeshSelection s;
        s.VertexIndex.resize((size_t)nv); s.TriangleIndex.resize((size_t)nt); s.Triangles.resize((size_t)nt * 3);
        s.Vertices.resize((size_t)nv); s.Colors.resize((size_t)nv);
        Check(sdfk_trimesh_select(h_, k.data(), s.VertexIndex.data(), s.TriangleIndex.data(), s.Triangles.data(), &s.Vertices.data()->X,
                                  &s.Colors.data()->X, &kv, &kt));
        s.VertexIndex.resize((size_t)kv); s.Vertices.resize((size_t)kv); s.Colors.resize((size_t)kv);
        s.TriangleIndex.resize((size_t)kt); s.Triangles.resize((size_t)kt * 3);
        return s;
    }
    // The neighbours of every vertex and the boundary bytes (sdfk_trimesh_adjacency); made once per handle and kept on it.
    MeshAdjacency Adjacency() const
    {
        MeshAdjacency a;
        int64_t n = 0;
        Check(sdfk_trimesh_adjacency(h_, nullptr, nullptr, nullptr, &n));
        a.Start.resize((size_t)nv_ + 1); a.Neighbors.resize((size_t)n); a.Boundary.resize((size_t)nv_);
        Check(sdfk_trimesh_adjacency(h_, a.Start.data(), a.Neighbors.data(), a.Boundary.data(), nullptr));
        return a;
    }
    // The positions after `iterations` iterations of Taubin's lambda | mu smoothing (sdfk_trimesh_smooth: one stated function of
    // the mesh and the arguments).  An iteration is a step with lambda, then, if mu != 0, a step with mu.  pinBoundary: the
    // vertices of edges with one triangle side stay.  This handle is not changed: its queries still see the old positions.
    std::vector<Vector3> Smooth(int iterations, float lambda = 0.5f, float mu = -0.53f, bool pinBoundary = true) const
    {
        std::vector<Vector3> out((size_t)nv_);
        Check(sdfk_trimesh_smooth(h_, iterations, lambda, mu, pinBoundary ? SDFK_TRIMESH_SMOOTH_PIN_BOUNDARY : 0, &out.data()->X));
        return out;
    }
    // Area-weighted unit vertex normals from the geometry (sdfk_trimesh_vertex_normals), zeros at a vertex without a triangle that
    // has an area.  positions: one per vertex, in place of the handle's own (the output of Smooth, say); empty: the handle's.
    std::vector<Vector3> VertexNormals(const std::vector<Vector3>& positions = {}, bool flip = false) const
    {
        if (!positions.empty() && (int64_t)positions.size() != nv_) throw std::invalid_argument("one position per vertex (positions)");
        std::vector<Vector3> out((size_t)nv_);
        Check(sdfk_trimesh_vertex_normals(h_, positions.empty() ? nullptr : &positions.data()->X, flip ? SDFK_TRIMESH_NORMALS_FLIP : 0,
                                          &out.data()->X));
        return out;
    }
    // The mesh with the vertices of equal position made one (sdfk_trimesh_weld: one stated function of the mesh and the
    // arguments).  tolerance 0: equal as values (-0 equals +0); > 0: the cell of a lattice of that size anchored at the origin --
    // two vertices closer than the tolerance on opposite sides of a cell face do not weld.  Triangles that become
    // index-degenerate and representatives no kept triangle names are dropped unless the flags keep them.  This handle is not changed.
    MeshWeld Weld(float tolerance = 0.0f, bool keepDegenerate = false, bool keepUnreferenced = false) const
    {
        MeshWeld w;
        int64_t kv = 0, kt = 0, stats[4] = {0, 0, 0, 0};
        w.VertexMap.resize((size_t)nv_); w.VertexIndex.resize((size_t)nv_); w.TriangleIndex.resize((size_t)nt_); w.Triangles.resize((size_t)nt_ * 3);
        w.Vertices.resize((size_t)nv_); w.Colors.resize((size_t)nv_);
        Check(sdfk_trimesh_weld(h_, tolerance, (keepDegenerate ? SDFK_WELD_KEEP_DEGENERATE : 0) | (keepUnreferenced ? SDFK_WELD_KEEP_UNREFERENCED : 0),
                                w.VertexMap.data(), w.VertexIndex.data(), w.TriangleIndex.data(), w.Triangles.data(), &w.Vertices.data()->X,
                                &w.Colors.data()->X, &kv, &kt, stats));
        w.VertexIndex.resize((size_t)kv); w.Vertices.resize((size_t)kv); w.Colors.resize((size_t)kv);
        w.TriangleIndex.resize((size_t)kt); w.Triangles.resize((size_t)kt * 3);
        w.Merged = stats[0]; w.DegenerateDropped = stats[1]; w.UnreferencedDropped = stats[2]; w.Passes = stats[3];
        return w;
    }
    // The mesh made smaller by vertex clustering (sdfk_trimesh_simplify: one stated function of the mesh and the arguments): the
    // vertices of one cell of the lattice of size cellSize become one made vertex; triangles that become index-degenerate are
    // dropped, and of those that come to share a vertex set `duplicates` decides.  This handle is not changed.
    MeshSimplify Simplify(float cellSize, SimplifyPlacement placement = SimplifyPlacement::Quadric,
                          SimplifyDuplicates duplicates = SimplifyDuplicates::One) const
    {
        MeshSimplify w;
        int64_t kv = 0, kt = 0, stats[6] = {0, 0, 0, 0, 0, 0};
        w.VertexMap.resize((size_t)nv_); w.VertexIndex.resize((size_t)nv_); w.TriangleIndex.resize((size_t)nt_); w.Triangles.resize((size_t)nt_ * 3);
        w.Vertices.resize((size_t)nv_); w.Colors.resize((size_t)nv_);
        Check(sdfk_trimesh_simplify(h_, cellSize, (int32_t)placement, (int32_t)duplicates, w.VertexMap.data(), w.VertexIndex.data(),
                                    w.TriangleIndex.data(), w.Triangles.data(), &w.Vertices.data()->X, &w.Colors.data()->X, &kv, &kt, stats));
        w.VertexIndex.resize((size_t)kv); w.Vertices.resize((size_t)kv); w.Colors.resize((size_t)kv);
        w.TriangleIndex.resize((size_t)kt); w.Triangles.resize((size_t)kt * 3);
        w.Merged = stats[0]; w.DegenerateDropped = stats[1]; w.DuplicatesDropped = stats[2]; w.UnreferencedDropped = stats[3]; w.Passes = stats[4];
        w.QuadricFallbacks = stats[5];
        return w;
    }
    // The first hit of every ray origin + t direction, tMin <= t <= tMax (sdfk_trimesh_raycast: one stated function of the mesh, the
    // rays and the range; the watertight ray-triangle test in binary64, ties to the lowest triangle index).  Directions need not be
    // unit vectors; one origin may be given for all directions.  A ray with a NaN or infinite component or a zero direction is a miss.
    MeshRayHits RayCast(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin = 0.0f, float tMax = INFINITY) const
    {
        MeshRayHits r;
        Rays(origins, directions, r.Origins, r.Directions);
        const size_t n = r.Directions.size();
        r.Triangles.resize(n); r.Distances.resize(n); r.Weights.resize(n);
        Check(sdfk_trimesh_raycast(h_, n ? &r.Origins.data()->X : nullptr, n ? &r.Directions.data()->X : nullptr, (int64_t)n, tMin, tMax, 0,
                                   r.Triangles.data(), r.Distances.data(), n ? &r.Weights.data()->X : nullptr));
        return r;
    }
    // Whether anything is hit within the range, per ray (SDFK_RAY_ANY_HIT: the search stops at the first hit it meets).
    std::vector<bool> Occluded(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin = 0.0f, float tMax = INFINITY) const
    {
        std::vector<Vector3> o, d;
        Rays(origins, directions, o, d);
        std::vector<int32_t> tri(d.size());
        Check(sdfk_trimesh_raycast(h_, d.empty() ? nullptr : &o.data()->X, d.empty() ? nullptr : &d.data()->X, (int64_t)d.size(), tMin, tMax,
                                   SDFK_RAY_ANY_HIT, tri.data(), nullptr, nullptr));
        std::vector<bool> out(d.size());
        for (size_t i = 0; i < d.size(); i++) out[i] = tri[i] >= 0;
        return out;
    }
    // The generalized winding number of every point (sdfk_trimesh_winding: one stated function of the mesh, the point and beta): on
    // a closed, consistently oriented mesh 0 outside and +1 or -1 inside, 2 where closed pieces overlap, 0 in a cavity; smooth where
    // the mesh is open; NaN for a point with a NaN or infinite coordinate.  Clusters of triangles farther than beta times their
    // radius are replaced by their first-order term; beta = INFINITY sums every triangle.  The hierarchy is made by the handle's
    // first call and kept.
    std::vector<float> WindingNumber(const std::vector<Vector3>& points, float beta = DefaultWindingBeta) const
    {
        std::vector<float> w(points.size());
        Check(sdfk_trimesh_winding(h_, points.empty() ? nullptr : &points.data()->X, (int64_t)points.size(), beta, w.data(), nullptr));
        return w;
    }
    // Whether each point is inside: |winding number| > 1/2, decided in binary64 before the rounding to float.  Independent of which
    // way the normals point; the union of overlapping closed pieces; holes are capped by the 1/2 level set.
    std::vector<bool> Contains(const std::vector<Vector3>& points, float beta = DefaultWindingBeta) const
    {
        std::vector<uint8_t> in(points.size());
        Check(sdfk_trimesh_winding(h_, points.empty() ? nullptr : &points.data()->X, (int64_t)points.size(), beta, nullptr, in.data()));
        return std::vector<bool>(in.begin(), in.end());
    }
    // The mesh as one camera sees it (sdfk_trimesh_render), with RayMarcher's own camera, lens defaults, light and sky: Render is
    // Lambert-shaded (vertex colours blended; a mesh without is white), RenderDepth the distance along every pixel's ray (+inf: the
    // sky), RenderTriangles the triangle every pixel sees (-1: the sky).  Defined after RayMarcher, whose camera they use.
    inline Vec3Data Render(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees = 60.0f, float nearPlaneDistance = 1.0f,
                           float farPlaneDistance = 100.0f) const;
    inline FloatData RenderDepth(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees = 60.0f,
                                 float nearPlaneDistance = 1.0f, float farPlaneDistance = 100.0f) const;
    inline std::vector<int32_t> RenderTriangles(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees = 60.0f,
                                                float nearPlaneDistance = 1.0f, float farPlaneDistance = 100.0f) const;
    // triangles of non-zero sampling weight and the total weight (the largest triangle has 2^32), as the last SamplePoints read them
    int64_t SampledTriangles() const { return sampleStats_[0]; }
    int64_t SampleTotalWeight() const { return sampleStats_[1]; }
    sdfk_trimesh* Handle() const { return h_; }

private:
    static bool AnyNonZero(const std::vector<Vector3>& c)
    {
        for (const Vector3& x : c) if (x.X != 0 || x.Y != 0 || x.Z != 0) return true;
        return false;
    }
    void Counts(int64_t* nv, int64_t* nt) const { *nv = nv_; *nt = nt_; }
    static void Rays(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, std::vector<Vector3>& o, std::vector<Vector3>& d)
    {
        if (origins.size() != directions.size() && origins.size() != 1) throw std::invalid_argument("one origin per direction, or one for all");
        d = directions;
        if (origins.size() == directions.size()) o = origins;
        else o.assign(directions.size(), origins[0]);
    }
    inline void RenderImages(int width, int height, const Matrix4x4& view, float fov, float nearp, float farp, float* depth, float* rgb,
                             int32_t* triangle) const;
    sdfk_trimesh* h_ = nullptr;
    bool hasColors_ = false;
    int64_t nv_ = 0, nt_ = 0;
    mutable int64_t sampleStats_[2] = {0, 0};
};

inline MeshSamples Mesh::SamplePoints(int64_t n, uint64_t seed, bool stratified) const { return MeshSdf(*this).SamplePoints(n, seed, stratified); }
inline MeshRayHits Mesh::RayCast(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin, float tMax) const
{
    return MeshSdf(*this).RayCast(origins, directions, tMin, tMax);
}
inline std::vector<bool> Mesh::Occluded(const std::vector<Vector3>& origins, const std::vector<Vector3>& directions, float tMin, float tMax) const
{
    return MeshSdf(*this).Occluded(origins, directions, tMin, tMax);
}
inline std::vector<float> Mesh::WindingNumber(const std::vector<Vector3>& points, float beta) const
{
    return MeshSdf(*this).WindingNumber(points, beta < 0 ? DefaultWindingBeta : beta);
}
inline std::vector<bool> Mesh::Contains(const std::vector<Vector3>& points, float beta) const
{
    return MeshSdf(*this).Contains(points, beta < 0 ? DefaultWindingBeta : beta);
}
inline MeshComponents Mesh::Components() const { return MeshSdf(*this).Components(); }
inline MeshTopology Mesh::Topology() const { return MeshSdf(*this).Topology(); }
namespace detail {
inline Mesh SelectedMesh(const Mesh& from, const MeshSdf& sdf, const std::vector<bool>& keep)
{
    MeshSelection s = sdf.Select(keep);
    Mesh m;
    m.Min = m.Max = Vector3(0, 0, 0);
    if (s.VertexIndex.empty()) return m;
    m.Normals.resize(s.VertexIndex.size());
    for (size_t i = 0; i < s.VertexIndex.size(); i++)
        m.Normals[i] = (size_t)s.VertexIndex[i] < from.Normals.size() ? from.Normals[(size_t)s.VertexIndex[i]] : Vector3(0, 0, 0);
    m.Vertices = std::move(s.Vertices); m.Colors = std::move(s.Colors); m.Triangles = std::move(s.Triangles);
    m.Min = m.Max = m.Vertices[0];
    for (const Vector3& v : m.Vertices) {   // Measure (Mesh.cs:30-45)
        m.Min = Vector3(std::min(m.Min.X, v.X), std::min(m.Min.Y, v.Y), std::min(m.Min.Z, v.Z));
        m.Max = Vector3(std::max(m.Max.X, v.X), std::max(m.Max.Y, v.Y), std::max(m.Max.Z, v.Z));
    }
    return m;
}
// The vertex normals of `positions` (empty: the handle's own) on the side of `present`: flipped iff more vertices have a negative
// dot product ((x x' + y y') + z z' in binary64) with their present normal than a positive one.
inline std::vector<Vector3> NormalsOnTheSideOf(const MeshSdf& sdf, const std::vector<Vector3>& positions, const std::vector<Vector3>& present)
{
    std::vector<Vector3> n = sdf.VertexNormals(positions);
    if (present.size() != n.size()) return n;
    int64_t pos = 0, neg = 0;
    for (size_t i = 0; i < n.size(); i++) {
        const double d = ((double)n[i].X * (double)present[i].X + (double)n[i].Y * (double)present[i].Y) + (double)n[i].Z * (double)present[i].Z;
        if (d > 0) pos++;
        if (d < 0) neg++;
    }
    return neg > pos ? sdf.VertexNormals(positions, true) : n;
}
inline void Measure(Mesh& m)   // Mesh.cs:30-45
{
    m.Min = m.Max = m.Vertices.empty() ? Vector3(0, 0, 0) : m.Vertices[0];
    for (const Vector3& v : m.Vertices) {
        m.Min = Vector3(std::min(m.Min.X, v.X), std::min(m.Min.Y, v.Y), std::min(m.Min.Z, v.Z));
        m.Max = Vector3(std::max(m.Max.X, v.X), std::max(m.Max.Y, v.Y), std::max(m.Max.Z, v.Z));
    }
}
}  // namespace detail
inline Mesh Mesh::Smooth(int iterations, float lambda, float mu, bool pinBoundary, bool normals) const
{
    MeshSdf sdf(*this);
    Mesh m;
    m.Vertices = sdf.Smooth(iterations, lambda, mu, pinBoundary);
    m.Colors = Colors; m.Triangles = Triangles;
    m.Normals = normals ? detail::NormalsOnTheSideOf(sdf, m.Vertices, Normals) : Normals;
    detail::Measure(m);
    return m;
}
inline Mesh Mesh::RecomputeNormals() const
{
    Mesh m = *this;
    m.Normals = detail::NormalsOnTheSideOf(MeshSdf(*this), {}, Normals);
    return m;
}
inline Mesh Mesh::RecomputeNormals(bool flip) const
{
    Mesh m = *this;
    m.Normals = MeshSdf(*this).VertexNormals({}, flip);
    return m;
}
inline Mesh Mesh::Weld(float tolerance, bool normals) const
{
    MeshWeld w = MeshSdf(*this).Weld(tolerance);
    Mesh m;
    m.Min = m.Max = Vector3(0, 0, 0);
    if (w.VertexIndex.empty()) return m;
    m.Normals.resize(w.VertexIndex.size());
    for (size_t i = 0; i < w.VertexIndex.size(); i++)
        m.Normals[i] = (size_t)w.VertexIndex[i] < Normals.size() ? Normals[(size_t)w.VertexIndex[i]] : Vector3(0, 0, 0);
    m.Vertices = std::move(w.Vertices); m.Colors = std::move(w.Colors); m.Triangles = std::move(w.Triangles);
    if (normals) m.Normals = detail::NormalsOnTheSideOf(MeshSdf(m.Vertices, m.Triangles), {}, m.Normals);
    detail::Measure(m);
    return m;
}
inline Mesh Mesh::Simplify(float cellSize, SimplifyPlacement placement, SimplifyDuplicates duplicates, bool normals) const
{
    MeshSimplify w = MeshSdf(*this).Simplify(cellSize, placement, duplicates);
    Mesh m;
    m.Min = m.Max = Vector3(0, 0, 0);
    if (w.VertexIndex.empty()) return m;
    m.Normals.resize(w.VertexIndex.size());
    for (size_t i = 0; i < w.VertexIndex.size(); i++)
        m.Normals[i] = (size_t)w.VertexIndex[i] < Normals.size() ? Normals[(size_t)w.VertexIndex[i]] : Vector3(0, 0, 0);
    m.Vertices = std::move(w.Vertices); m.Colors = std::move(w.Colors); m.Triangles = std::move(w.Triangles);
    if (normals) m.Normals = detail::NormalsOnTheSideOf(MeshSdf(m.Vertices, m.Triangles), {}, m.Normals);
    detail::Measure(m);
    return m;
}
inline Mesh Mesh::Concat(const std::vector<Mesh>& meshes)
{
    Mesh m;
    for (const Mesh& p : meshes) {
        const size_t base = m.Vertices.size(), n = p.Vertices.size();
        if (base + n >= (size_t(1) << 31)) throw std::invalid_argument("2^31 vertices or more (Concat)");
        m.Vertices.insert(m.Vertices.end(), p.Vertices.begin(), p.Vertices.end());
        for (size_t i = 0; i < n; i++) {
            m.Colors.push_back(p.Colors.size() == n ? p.Colors[i] : Vector3(0, 0, 0));
            m.Normals.push_back(p.Normals.size() == n ? p.Normals[i] : Vector3(0, 0, 0));
        }
        for (int32_t t : p.Triangles) m.Triangles.push_back(t + (int32_t)base);
    }
    detail::Measure(m);
    return m;
}
inline Mesh Mesh::SelectComponents(const std::vector<bool>& keep) const { return detail::SelectedMesh(*this, MeshSdf(*this), keep); }
inline Mesh Mesh::RemoveSmallComponents(int64_t minTriangles, float minAreaFraction) const
{
    MeshSdf sdf(*this);
    const MeshComponents c = sdf.Components();
    int64_t total = 0;
    for (int64_t w : c.AreaWeights) total += w;
    std::vector<bool> keep((size_t)c.Count);
    for (size_t i = 0; i < keep.size(); i++)
        keep[i] = c.Triangles[i] >= minTriangles && (double)c.AreaWeights[i] >= (double)minAreaFraction * (double)total;
    return detail::SelectedMesh(*this, sdf, keep);
}
inline Mesh Mesh::LargestComponent() const
{
    MeshSdf sdf(*this);
    const MeshComponents c = sdf.Components();
    size_t best = 0;
    for (size_t i = 1; i < (size_t)c.Count; i++)
        if (c.AreaWeights[i] != c.AreaWeights[best] ? c.AreaWeights[i] > c.AreaWeights[best] : c.Triangles[i] > c.Triangles[best]) best = i;
    std::vector<bool> keep((size_t)c.Count, false);
    if (c.Count) keep[best] = true;
    return detail::SelectedMesh(*this, sdf, keep);
}

struct FloatData {   // VectorData.cs:137-280; indexer is (x, y)
    int Width = 0, Height = 0;
    std::vector<float> Values;
    float operator()(int x, int y) const { return Values[(size_t)y * Width + x]; }
    void SaveDepthTga(const std::string& path, float nearv, float farv) const   // VectorData.cs:244-279
    {
        std::ofstream w(path, std::ios::binary);
        WriteTgaHeader(w, 3, Width, Height, 8);
        for (float v : Values) {
            const unsigned char b = v >= farv ? 0 : (v <= nearv ? 255 : (unsigned char)(255.0f * (farv - v) / (farv - nearv)));
            w.put((char)b);
        }
    }
};
struct Vec3Data {    // VectorData.cs:343-620
    int Width = 0, Height = 0;
    std::vector<float> Values;   // 3 per pixel
    Vector3 operator()(int x, int y) const { const float* p = &Values[((size_t)y * Width + x) * 3]; return {p[0], p[1], p[2]}; }
    void SaveTga(const std::string& path) const   // VectorData.cs:570-619: 24-bit B, G, R, channel * 255 truncated and clamped
    {
        std::ofstream w(path, std::ios::binary);
        WriteTgaHeader(w, 2, Width, Height, 24);
        for (size_t k = 0; k + 2 < Values.size(); k += 3)
            for (int c = 2; c >= 0; c--) {
                const float v = Values[k + c] * 255.0f;
                w.put((char)(v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (unsigned char)v)));
            }
    }
};

class RayMarcher {   // RayMarcher.cs:7-43: same constructor, properties and defaults
public:
    static constexpr float DefaultNearPlaneDistance = 1.0f, DefaultFarPlaneDistance = 100.0f, DefaultVerticalFieldOfViewDegrees = 60.0f;
    static constexpr int DefaultDepthIterations = 40;
    Matrix4x4 ViewTransform = Matrix4x4::CreateLookAt(Vector3(0, 0, 5), Vector3(0, 0, 0), Vector3(0, 1, 0));
    float NearPlaneDistance = DefaultNearPlaneDistance, FarPlaneDistance = DefaultFarPlaneDistance;
    float VerticalFieldOfViewDegrees = DefaultVerticalFieldOfViewDegrees;
    int DepthIterations = DefaultDepthIterations;
    RayMarcher(int width, int height, Sdf sdf, int /*batchSize*/ = 2048, int /*maxDegreeOfParallelism*/ = -1) : w_(width), h_(height), sdf_(std::move(sdf)) {}
    Vec3Data Render() const { Vec3Data d; d.Width = w_; d.Height = h_; d.Values.resize((size_t)w_ * h_ * 3); Run(nullptr, d.Values.data()); return d; }
    FloatData RenderDepth() const { FloatData d; d.Width = w_; d.Height = h_; d.Values.resize((size_t)w_ * h_); Run(d.Values.data(), nullptr); return d; }

    // host part of GetCameraRays (RayMarcher.cs:97-112): the camera position and the inverse view-projection sdfk_raymarch takes
    void Camera(float pos[3], Matrix4x4& vpi) const { CameraOf(ViewTransform, w_, h_, VerticalFieldOfViewDegrees, NearPlaneDistance, FarPlaneDistance, pos, vpi); }
    // (static: MeshSdf's renders use the same camera and have no Sdf to construct a RayMarcher with)
    static void CameraOf(const Matrix4x4& view, int width, int height, float verticalFieldOfViewDegrees, float nearPlane, float farPlane, float pos[3],
                         Matrix4x4& vpi)
    {
        Matrix4x4 cam;
        Matrix4x4::Invert(view, cam);
        pos[0] = ((0.0f * cam.M[0][0] + 0.0f * cam.M[1][0]) + 0.0f * cam.M[2][0]) + cam.M[3][0];
        pos[1] = ((0.0f * cam.M[0][1] + 0.0f * cam.M[1][1]) + 0.0f * cam.M[2][1]) + cam.M[3][1];
        pos[2] = ((0.0f * cam.M[0][2] + 0.0f * cam.M[1][2]) + 0.0f * cam.M[2][2]) + cam.M[3][2];
        const Matrix4x4 proj = Matrix4x4::CreatePerspectiveFieldOfView(verticalFieldOfViewDegrees * 3.14159274f / 180.0f, (float)width / (float)height,
                                                                       nearPlane, farPlane);
        Matrix4x4::Invert(view * proj, vpi);
    }

private:
    void Run(float* depth, float* rgb) const
    {
        float pos[3];
        Matrix4x4 vpi;
        Camera(pos, vpi);
        EnsureInit();
        Check(sdfk_raymarch(sdf_.Program(), w_, h_, pos, &vpi.M[0][0], NearPlaneDistance, FarPlaneDistance, DepthIterations, depth, rgb));
    }
    int w_, h_;
    Sdf sdf_;
};

// ---- MeshSdf's and Mesh's renders: RayMarcher's camera, sdfk_trimesh_render's images ---------------------------------------
inline void MeshSdf::RenderImages(int width, int height, const Matrix4x4& view, float fov, float nearp, float farp, float* depth, float* rgb,
                                  int32_t* triangle) const
{
    float pos[3];
    Matrix4x4 vpi;
    RayMarcher::CameraOf(view, width, height, fov, nearp, farp, pos, vpi);
    Check(sdfk_trimesh_render(h_, width, height, pos, &vpi.M[0][0], nearp, farp, depth, rgb, triangle));
}
inline Vec3Data MeshSdf::Render(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees, float nearPlaneDistance,
                                float farPlaneDistance) const
{
    Vec3Data d;
    d.Width = width; d.Height = height;
    d.Values.resize((size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0) * 3);
    RenderImages(width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, nullptr, d.Values.data(), nullptr);
    return d;
}
inline FloatData MeshSdf::RenderDepth(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees, float nearPlaneDistance,
                                      float farPlaneDistance) const
{
    FloatData d;
    d.Width = width; d.Height = height;
    d.Values.resize((size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0));
    RenderImages(width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, d.Values.data(), nullptr, nullptr);
    return d;
}
inline std::vector<int32_t> MeshSdf::RenderTriangles(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees,
                                                     float nearPlaneDistance, float farPlaneDistance) const
{
    std::vector<int32_t> t((size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0));
    RenderImages(width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, nullptr, nullptr, t.data());
    return t;
}
inline Vec3Data Mesh::ToImage(int width, int height, const Matrix4x4& viewTransform, float verticalFieldOfViewDegrees, float nearPlaneDistance,
                              float farPlaneDistance) const
{
    return MeshSdf(*this).Render(width, height, viewTransform, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance);
}
inline Vec3Data Mesh::ToImage(int width, int height, Vector3 cameraPosition, Vector3 cameraTarget, Vector3 cameraUp, float verticalFieldOfViewDegrees,
                              float nearPlaneDistance, float farPlaneDistance) const
{
    return ToImage(width, height, Matrix4x4::CreateLookAt(cameraPosition, cameraTarget, cameraUp), verticalFieldOfViewDegrees, nearPlaneDistance,
                   farPlaneDistance);
}

// ---- depth frames into volumes and points (include/sdfkit_hip.h, "Depth images: fusion and unprojection") ------------------
// A depth frame is what RayMarcher::RenderDepth and MeshSdf::RenderDepth make: the distance along every pixel's ray, +inf where
// nothing was seen.  DepthFusion averages frames with poses into a volume of truncated signed distances (Curless & Levoy 1996).
// The unseen convention: a voxel no frame has observed keeps `unseen`.  With the default -truncation and carve (a pixel that saw
// nothing within depthMax frees the space along its ray) unseen space is solid and seen-empty space is free, so a fully scanned
// object meshes watertight; unseen = +truncation without carving is the classic open surface, with a spurious sheet one
// truncation behind every observed surface.
struct DepthFusionStats { int64_t Updated = 0, Surface = 0, First = 0, ValidPixels = 0; };

class DepthFusion {
public:
    float Truncation, Unseen, MaxWeight;
    bool Carve;
    int Frames = 0;
    Voxels Values, Weights;
    // unseen NAN: -truncation
    DepthFusion(Vector3 min, Vector3 max, int nx, int ny, int nz, float truncation, float unseen = NAN, bool carve = true, float maxWeight = INFINITY)
        : Truncation(truncation), Unseen(unseen != unseen ? -truncation : unseen), MaxWeight(maxWeight), Carve(carve), Values(min, max, nx, ny, nz),
          Weights(min, max, nx, ny, nz)
    {
        const std::vector<float> fill((size_t)nx * ny * nz, Unseen), zero((size_t)nx * ny * nz, 0.0f);
        Values.Ensure(false);
        Weights.Ensure(false);
        Check(sdfk_volume_upload(Values.h_, fill.data(), nullptr));
        Check(sdfk_volume_upload(Weights.h_, zero.data(), nullptr));
    }
    // One frame into the average, seen by the camera it was rendered with (RayMarcher's lens and defaults).  depthMin / depthMax:
    // the range of depths that are observations (NAN: the near / the far plane).
    DepthFusion& Integrate(const FloatData& depth, const Matrix4x4& viewTransform, float weight = 1.0f, float depthMin = NAN, float depthMax = NAN,
                           DepthFusionStats* stats = nullptr, float verticalFieldOfViewDegrees = 60.0f, float nearPlaneDistance = 1.0f,
                           float farPlaneDistance = 100.0f);
    DepthFusion& Integrate(const FloatData& depth, Vector3 cameraPosition, Vector3 cameraTarget, Vector3 cameraUp, float weight = 1.0f,
                           float depthMin = NAN, float depthMax = NAN, DepthFusionStats* stats = nullptr, float verticalFieldOfViewDegrees = 60.0f,
                           float nearPlaneDistance = 1.0f, float farPlaneDistance = 100.0f)
    {
        return Integrate(depth, Matrix4x4::CreateLookAt(cameraPosition, cameraTarget, cameraUp), weight, depthMin, depthMax, stats,
                         verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance);
    }
    // From a depth image in device memory, queued on the library stream: the camera position and the FORWARD view-projection
    // (ViewTransform x projection, the matrix whose inverse the renders take).
    DepthFusion& IntegrateDevice(const void* depthDev, int width, int height, const float cameraPosition[3], const Matrix4x4& viewProjection,
                                 float depthMin, float depthMax, float weight = 1.0f, DepthFusionStats* stats = nullptr)
    {
        const sdfk_fusion_params prm{Truncation, depthMin, depthMax, weight, MaxWeight, Carve ? SDFK_FUSE_CARVE_BEYOND : 0};
        int64_t st[4] = {0, 0, 0, 0};
        Check(sdfk_volume_integrate_depth_device(Handle(Values), Handle(Weights), depthDev, width, height, cameraPosition, &viewProjection.M[0][0], &prm,
                                                 stats ? st : nullptr));
        Done(stats, st);
        return *this;
    }
    Voxels& ToVoxels() { return Values; }
    // The surface of the fused volume; redistance: through Voxels::Redistance first, which makes distances of the projective,
    // clamped values.
    inline Mesh ToMesh(float isoValue = 0.0f, bool redistance = true);

private:
    static sdfk_volume* Handle(Voxels& v)
    {
        sdfk_volume* h = v.Sync();   // (host edits go up first, as everywhere)
        v.values_.clear();
        v.version_++;
        return h;
    }
    void Done(DepthFusionStats* stats, const int64_t st[4])
    {
        Frames++;
        if (stats) { stats->Updated = st[0]; stats->Surface = st[1]; stats->First = st[2]; stats->ValidPixels = st[3]; }
    }
};

struct DepthPoints {
    std::vector<Vector3> Points, Colors;   // Colors: empty without rgb
    std::vector<int32_t> Pixels;           // j * width + i of every point
};

inline DepthFusion& DepthFusion::Integrate(const FloatData& depth, const Matrix4x4& viewTransform, float weight, float depthMin, float depthMax,
                                           DepthFusionStats* stats, float verticalFieldOfViewDegrees, float nearPlaneDistance, float farPlaneDistance)
{
    float pos[3];
    Matrix4x4 vpi;
    RayMarcher::CameraOf(viewTransform, depth.Width, depth.Height, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, pos, vpi);
    const Matrix4x4 vp = viewTransform * Matrix4x4::CreatePerspectiveFieldOfView(verticalFieldOfViewDegrees * 3.14159274f / 180.0f,
                                                                                  (float)depth.Width / (float)depth.Height, nearPlaneDistance,
                                                                                  farPlaneDistance);
    const sdfk_fusion_params prm{Truncation, depthMin != depthMin ? nearPlaneDistance : depthMin, depthMax != depthMax ? farPlaneDistance : depthMax,
                                 weight, MaxWeight, Carve ? SDFK_FUSE_CARVE_BEYOND : 0};
    int64_t st[4] = {0, 0, 0, 0};
    Check(sdfk_volume_integrate_depth(Handle(Values), Handle(Weights), depth.Values.data(), depth.Width, depth.Height, pos, &vp.M[0][0], &prm,
                                      stats ? st : nullptr));
    Done(stats, st);
    return *this;
}
inline Mesh DepthFusion::ToMesh(float isoValue, bool redistance)
{
    if (!redistance) return Values.ToMesh(isoValue);
    Voxels r = Values.Redistance(isoValue);
    return r.ToMesh(isoValue);
}

// A depth frame as points: camera + ray * depth for every pixel with depthMin <= depth <= depthMax (NAN: the near / the far
// plane), in pixel order -- for a frame MeshSdf::RenderDepth made, that render's hit points bit for bit.  rgb: the colours to gather.
inline DepthPoints DepthToPoints(const FloatData& depth, const Matrix4x4& viewTransform, const Vec3Data* rgb = nullptr, float depthMin = NAN,
                                 float depthMax = NAN, float verticalFieldOfViewDegrees = 60.0f, float nearPlaneDistance = 1.0f,
                                 float farPlaneDistance = 100.0f)
{
    float pos[3];
    Matrix4x4 vpi;
    RayMarcher::CameraOf(viewTransform, depth.Width, depth.Height, verticalFieldOfViewDegrees, nearPlaneDistance, farPlaneDistance, pos, vpi);
    const size_t n = (size_t)(depth.Width > 0 ? depth.Width : 0) * (size_t)(depth.Height > 0 ? depth.Height : 0);
    if (rgb && (rgb->Width != depth.Width || rgb->Height != depth.Height)) throw std::invalid_argument("SdfKit::DepthToPoints: rgb is not the depth image's size");
    DepthPoints out;
    out.Points.resize(n);
    out.Pixels.resize(n);
    if (rgb) out.Colors.resize(n);
    int64_t k = 0;
    EnsureInit();
    Check(sdfk_depth_unproject(depth.Values.data(), rgb ? rgb->Values.data() : nullptr, depth.Width, depth.Height, pos, &vpi.M[0][0],
                               depthMin != depthMin ? nearPlaneDistance : depthMin, depthMax != depthMax ? farPlaneDistance : depthMax,
                               n ? &out.Points[0].X : nullptr, rgb && n ? &out.Colors[0].X : nullptr, out.Pixels.data(), &k));
    out.Points.resize((size_t)k);
    out.Pixels.resize((size_t)k);
    if (rgb) out.Colors.resize((size_t)k);
    return out;
}
inline DepthPoints DepthToPoints(const FloatData& depth, Vector3 cameraPosition, Vector3 cameraTarget, Vector3 cameraUp, const Vec3Data* rgb = nullptr,
                                 float depthMin = NAN, float depthMax = NAN, float verticalFieldOfViewDegrees = 60.0f, float nearPlaneDistance = 1.0f,
                                 float farPlaneDistance = 100.0f)
{
    return DepthToPoints(depth, Matrix4x4::CreateLookAt(cameraPosition, cameraTarget, cameraUp), rgb, depthMin, depthMax, verticalFieldOfViewDegrees,
                         nearPlaneDistance, farPlaneDistance);
}

}  // namespace SdfKit
