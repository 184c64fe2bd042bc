// rm_api_errmodel.cpp -- C ABI: the frame error model of the SINR medium: parameters, refusals, host exports.
#include "rm_host.hpp"

using namespace rmh;

namespace rmh {

rm::EmDev em_dev(const rm_context *c)
{
    rm::EmDev d{};
    d.us_per_bit = c->em.us_per_bit;
    d.seed = c->em.seed;
    return d;
}

} // namespace rmh

static int em_validate(const rm_error_model *e)
{
    if (e->kind != RM_EM_NONE && e->kind != RM_EM_OQPSK_250K) return fail(RM_ERR_INVALID, "unknown error model kind");
    if (e->reserved != 0) return fail(RM_ERR_INVALID, "rm_error_model.reserved has to be 0");
    if (!(std::isfinite(e->us_per_bit) && e->us_per_bit > 0.0)) return fail(RM_ERR_INVALID, "us_per_bit has to be finite and > 0");
    return RM_OK;
}

extern "C" {

void rm_error_model_defaults(rm_error_model *e, int32_t kind)
{
    if (!e) return;
    e->kind = kind;
    e->reserved = 0;
    e->us_per_bit = 4.0;
    e->seed = 0;
}

int rm_set_error_model(rm_context *c, const rm_error_model *e)
{
    if (!c || !e) return fail(RM_ERR_INVALID, "NULL argument");
    if (!is_sinr(c)) return fail(RM_ERR_STATE, "the frame error model needs RM_MODEL_LOGDIST with RM_LD_SINR: only that medium has a link's sinr");
    RM_TRY(em_validate(e));
    if (e->kind != RM_EM_NONE) RM_TRY(graphs_refuse(c, "the error model's pass is not part of them"));
    RM_TRY(ev_flush_append(c)); // (the tick before was evaluated without the new model: its append does not wait for the next drain)
    ev_touch(c);
    c->em = *e;
    return RM_OK;
}

int rm_get_error_model(const rm_context *c, rm_error_model *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "NULL argument");
    *out = c->em;
    if (out->kind == RM_EM_NONE && !(out->us_per_bit > 0.0)) rm_error_model_defaults(out, RM_EM_NONE);
    return RM_OK;
}

double rm_error_model_psr(const rm_error_model *e, double sinr_db, int64_t air_us)
{
    if (!e) return 1.0;
    return rm::host_em_psr(e->kind, e->us_per_bit, sinr_db, air_us);
}

double rm_error_model_draw(const rm_error_model *e, int32_t src, int64_t start_us, int32_t dst)
{
    return rm::host_em_draw(e ? e->seed : 0, src, start_us, dst);
}

} // extern "C"
