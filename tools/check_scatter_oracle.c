/* tools/check_scatter_oracle.c — the oracle's own reflect, refract and Material::scatter (oracle/r1_oracle.c, static there) behind
 * three entry points, for tools/check_scatter_host.cpp.  Built by tests/test_scatter_host.py with the oracle's flags:
 *   gcc -O3 -std=gnu11 -mavx2 -mfma -ffp-contract=off -fno-fast-math -DR1_ORACLE_TU='"<root>/oracle/r1_oracle.c"' -c ...
 * Test infrastructure, never linked into the product. */
#include R1_ORACLE_TU

void r1so_reflect(const float v[3], const float n[3], float out[3])
{
    const v3 r = reflect(v3_from(v), v3_from(n));
    out[0] = r.x, out[1] = r.y, out[2] = r.z;
}

int r1so_refract(const float v[3], const float outward[3], float ni_over_nt, float out[3])
{
    v3 r = V(0, 0, 0);
    const int ok = refract(v3_from(v), v3_from(outward), ni_over_nt, &r);
    out[0] = r.x, out[1] = r.y, out[2] = r.z;
    return ok;
}

/* scatter() at a hit of a sphere with material (mat_type, mat_param): streams = {scalar, lane0 .. lane3}, advanced as scatter draws;
 * out = the scattered ray's (normalised) direction; returns scatter's result */
int r1so_scatter(int mat_type, float mat_param, const float d[3], const float p[3], const float n[3], uint32_t streams[5], float out[3])
{
    const uint8_t type = (uint8_t)mat_type;
    const float albedo = 0.5f;
    r1_scene sc;
    memset(&sc, 0, sizeof(sc));
    sc.count = 1;
    sc.mat_type = &type, sc.mat_param = &mat_param;
    sc.albedo_r = sc.albedo_g = sc.albedo_b = &albedo;
    tracer t;
    memset(&t, 0, sizeof(t));
    t.sc = &sc;
    t.st.scalar = streams[0];
    memcpy(t.st.lanes, streams + 1, sizeof(t.st.lanes));
    ray in;
    in.o = V(0, 0, 0), in.d = v3_from(d);
    hit_record rec;
    rec.t = 1, rec.p = v3_from(p), rec.normal = v3_from(n), rec.index = 0;
    v3 att;
    ray s;
    s.o = s.d = V(0, 0, 0);
    const int ok = scatter(&t, in, &rec, &att, &s);
    streams[0] = t.st.scalar;
    memcpy(streams + 1, t.st.lanes, sizeof(t.st.lanes));
    out[0] = s.d.x, out[1] = s.d.y, out[2] = s.d.z;
    return ok;
}
