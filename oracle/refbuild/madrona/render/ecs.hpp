/*
 * Stand-in for the engine's render ECS interface (test infrastructure only).
 *
 * A stub: it owns the storage the simulation source reads and writes -- the
 * finder output of each camera, the four raycast output buffers, a camera's
 * output row and an instance's species index -- and traces nothing.  The
 * lock-step driver writes finder hits and sensor rows into it from outside.
 */
#pragma once
#include "../standin.hpp"

namespace madrona::render {

struct RenderECSBridge;

struct Renderable {
    Entity renderEntity;
};
struct RenderCamera {
    Entity cameraEntity;
};
struct PerspectiveCameraData {
    uint32_t rowIDX;
    float fov;
    float zNear;
    math::Vector3 offset;
};
struct InstanceData {
    uint32_t speciesIDX;
};
struct FinderOutput {
    Entity hitEntity;
};
struct FinderOutputBuffer {
    FinderOutput out;
};

/* 32 bytes a row: the width the simulation source copies */
struct SemanticOutputBuffer { uint8_t px[32]; };
struct DepthOutputBuffer { uint8_t px[32]; };
struct PrevSemanticOutputBuffer { uint8_t px[32]; };
struct PrevDepthOutputBuffer { uint8_t px[32]; };

struct RaycastOutputArchetype : Archetype<SemanticOutputBuffer, DepthOutputBuffer, PrevSemanticOutputBuffer,
                                          PrevDepthOutputBuffer> {};
struct CameraArchetype : Archetype<PerspectiveCameraData, FinderOutputBuffer> {};
struct InstanceArchetype : Archetype<InstanceData> {};

namespace RenderingSystem {

/* called with each entity a view was attached to (the driver sets the output
 * row a new agent starts from) */
inline void (*&onAttachView())(Context &, Entity)
{
    static void (*fn)(Context &, Entity) = nullptr;
    return fn;
}
/* called with each entity made renderable */
inline void (*&onMakeRenderable())(Context &, Entity)
{
    static void (*fn)(Context &, Entity) = nullptr;
    return fn;
}

inline void registerTypes(ECSRegistry &registry, RenderECSBridge *)
{
    StateManager *sm = registry.stateManager();
    sm->addArchetype<RaycastOutputArchetype>((RaycastOutputArchetype *)nullptr, false);
    registry.registerArchetype<CameraArchetype>();
    registry.registerArchetype<InstanceArchetype>();
}

template <typename ContextT> void init(ContextT &, RenderECSBridge *) {}

template <typename ContextT> void makeEntityRenderable(ContextT &ctx, Entity e)
{
    ctx.template get<Renderable>(e).renderEntity = ctx.template makeEntity<InstanceArchetype>();
    if (onMakeRenderable()) onMakeRenderable()(ctx, e);
}

template <typename ContextT> void cleanupRenderableEntity(ContextT &ctx, Entity e)
{
    ctx.destroyEntity(ctx.template get<Renderable>(e).renderEntity);
}

template <typename ContextT>
void attachEntityToView(ContextT &ctx, Entity e, float fov, float z_near, const math::Vector3 &offset)
{
    Entity cam = ctx.template makeEntity<CameraArchetype>();
    PerspectiveCameraData &d = ctx.template get<PerspectiveCameraData>(cam);
    d.fov = fov;
    d.zNear = z_near;
    d.offset = offset;
    ctx.template get<FinderOutputBuffer>(cam).out.hitEntity = Entity::none();
    ctx.template get<RenderCamera>(e).cameraEntity = cam;
    if (onAttachView()) onAttachView()(ctx, e);
}

template <typename ContextT> void cleanupViewingEntity(ContextT &ctx, Entity e)
{
    ctx.destroyEntity(ctx.template get<RenderCamera>(e).cameraEntity);
}

template <typename BufferT, typename ContextT> void *getRenderOutput(ContextT &ctx, const RenderCamera &camera, uint32_t)
{
    return &ctx.template get<BufferT>(camera.cameraEntity);
}

inline void setupTasks(TaskGraphBuilder &, Span<const TaskGraph::NodeID>) {}

}  // namespace RenderingSystem
}  // namespace madrona::render
